"""GPU: the align step -- tmh_register_shifts / tmh_xcorr_plane through the
C-ABI and tmlibrary_amd.workflow.align -- against the numpy f64 literal of the
rule (tests/xcorr_literal.py).

Inputs: one seeded blob field (~1 blob per 400 px); target and reference are
two windows of it, so the edges are not cyclic; gain 1.1 on the target and
independent sigma = 8 noise on each.  On every case the literal's own plane
must hold its peak >= 1 % of the plane's span above everything outside the
peak's cyclic 3x3 neighbourhood (asserted first; a complex64 transform is
wrong by ~3e-7 of the span, five orders below).  Sparse small fields do not
always recover the planted shift, so the shifts are compared with the
literal's argmax, exactly.

Plane bound: |plane - literal| <= 4 x (numpy's complex64 form - literal) +
1e-7 of the span; the margin is for another radix order, the two-for-one
split and twiddle rounding, not for a wrong algorithm.

test_plane_per_geometry applies that bound at every class of launch geometry
the kernels' host code can pick (tests/align_cases.py); the batch tests pass
one chunk, one launch and one k_reg_sums launch; the sums tests rest on a
constant image's plane being exactly 0.0 only when its own sum reaches it.
"""
import os

import numpy as np
import pytest

import align_cases as ac
import xcorr_literal as xl
from oracle import corilla_oracle as orc
from tmlibrary_amd import hip

pytestmark = pytest.mark.gpu

MARGIN = 0.01
RATIO, FLOOR = 4.0, 1e-7

#: shape, (dy, dx), dtype -- what each shape is there for: see the table below
CASES = [
    ((30, 40), (3, -5), np.uint16),      # radix 2, 3 and 5 mixed
    ((30, 40), (-2, 0), np.uint8),
    ((48, 81), (-7, 4), np.uint16),      # 3^4
    ((64, 64), (0, 9), np.uint16),       # pure radix 2 (radix-4 passes)
    ((64, 64), (0, 0), np.uint8),
    ((125, 128), (11, 0), np.uint16),    # 5^3, and 2^7: a radix-2 pass after the radix-4 ones
    ((37, 53), (-4, -6), np.uint16),     # both axes padded and folded
    ((37, 53), (5, 3), np.uint8),
    ((96, 53), (5, 7), np.uint16),       # one axis padded
    ((53, 96), (-6, -2), np.uint16),     # the other one
    ((1, 64), (0, 6), np.uint16),        # degenerate axes
    ((64, 1), (-5, 0), np.uint16),
    ((270, 320), (-13, 12), np.uint16),  # the production factor mix at 1/8 scale
    ((270, 320), (6, 16), np.uint8),
    ((2160, 2560), (14, -9), np.uint16),  # one pair at full size
    ((1040, 1392), (-8, 15), np.uint16),  # one padded pair at full size
]


@pytest.fixture(scope="module")
def reg():
    from tmlibrary_amd import hip
    from tmlibrary_amd.workflow.align import registration
    hip.lib()
    return registration


def _checked_literal(t, r):
    """The literal's shift, after asserting the condition on its plane."""
    c = xl.plane(t, r)
    margin = xl.peak_margin(c)
    print("literal margin %.4f" % margin)
    assert margin >= MARGIN, "the case misses the 1 %% condition (margin %.4f): new seed" % margin
    return xl.shift_of_plane(c), c


@pytest.mark.parametrize("shape,planted,dtype", CASES,
                         ids=["%dx%d_%s_%d_%d" % (s[0], s[1], np.dtype(d).name, p[0], p[1])
                              for s, p, d in CASES])
def test_shift_equals_literal(reg, shape, planted, dtype):
    t, r = xl.blob_pair(shape, planted[0], planted[1], seed=7, dtype=dtype)
    want, _ = _checked_literal(t, r)
    got = reg.calculate_shift(t, r)
    print("planted", planted, "literal", want, "gpu", got)
    assert all(type(v) is int for v in got)
    assert got == want


@pytest.mark.parametrize("shape,lag", [((30, 40), (15, 20)), ((30, 40), (16, 21)),
                                       ((37, 53), (18, 26)), ((37, 53), (19, 27)),
                                       ((64, 64), (32, 32))])
def test_half_length_lag_maps_to_plus(reg, shape, lag):
    """A cyclic pair at a lag of exactly L / 2 gives +L / 2; one beyond, the
    negative lag."""
    _, r = xl.blob_pair(shape, 0, 0, seed=11)
    t = np.roll(r, (-lag[0], -lag[1]), axis=(0, 1))  # T[r, c] = R[r + lag], cyclic
    want = (xl.signed_lag(lag[0], shape[0]), xl.signed_lag(lag[1], shape[1]))
    assert xl.shift(t, r) == want
    assert reg.calculate_shift(t, r) == want
    if lag == (shape[0] // 2, shape[1] // 2):
        assert want == lag


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_identical_and_constant_images(reg, dtype):
    for shape in ((30, 40), (37, 53), (64, 64)):
        t, _ = xl.blob_pair(shape, 0, 0, seed=3, dtype=dtype)
        assert reg.calculate_shift(t, t.copy()) == (0, 0)
        a, b = np.full(shape, 9, dtype), np.full(shape, 200, dtype)
        assert reg.calculate_shift(a, b) == (0, 0)
        y, x, peak = reg.calculate_shifts(a, b, return_peak=True)
        assert (int(y[0]), int(x[0]), float(peak[0])) == (0, 0, 0.0)


def _batch(shape=(64, 80), dtype=np.uint16):
    shifts = [(3, -5), (0, 0), (-7, 2), (9, 9), (-1, -12), (4, 0), (0, -3)]
    ref_of = np.array([0, 2, 1, 1, 0, 2, 2], np.int32)
    refs = np.stack([xl.blob_pair(shape, 0, 0, seed=40 + k, dtype=dtype)[1] for k in range(3)])
    targets = np.stack([xl.blob_pair(shape, dy, dx, seed=40 + int(k), dtype=dtype)[0]
                        for (dy, dx), k in zip(shifts, ref_of)])
    return targets, refs, ref_of


@pytest.mark.parametrize("dtype", [np.uint16, np.uint8])
def test_batch_equals_single_pairs(reg, dtype):
    """7 targets against 3 references in one call = the pairs one at a time =
    the literal; device-resident and host-pointer entry points agree."""
    import torch
    targets, refs, ref_of = _batch(dtype=dtype)
    want = [_checked_literal(targets[i], refs[ref_of[i]])[0] for i in range(len(targets))]
    assert len(set(want)) >= 5  # different shifts per pair
    y, x, peak = reg.calculate_shifts(targets, refs, ref_of, return_peak=True)
    assert y.dtype == np.int32 and x.dtype == np.int32 and y.shape == (7,)
    assert list(zip(y.tolist(), x.tolist())) == want
    singles = [reg.calculate_shifts(targets[i], refs[ref_of[i]], return_peak=True)
               for i in range(len(targets))]
    assert [(int(s[0][0]), int(s[1][0])) for s in singles] == want
    assert np.array_equal(np.array([s[2][0] for s in singles]), peak)
    store = np.int16 if dtype == np.uint16 else np.uint8
    dt = torch.from_numpy(targets.view(store)).cuda()
    dr = torch.from_numpy(refs.view(store)).cuda()
    dy, dx, dpeak = reg.calculate_shifts(dt, dr, ref_of, return_peak=True)
    assert np.array_equal(dy, y) and np.array_equal(dx, x) and np.array_equal(dpeak, peak)


@pytest.mark.parametrize("shape,planted", [((30, 40), (3, -5)), ((37, 53), (-4, -6)),
                                           ((270, 320), (-13, 12))])
def test_plane_against_literal(reg, shape, planted):
    t, r = xl.blob_pair(shape, planted[0], planted[1], seed=7)
    _, c = _checked_literal(t, r)
    got = reg.xcorr_plane(t, r)
    assert got.dtype == np.float32 and got.shape == shape
    span = float(c.max() - c.min())
    err = float(np.abs(got - c).max())
    ref = float(np.abs(xl.plane_c64(t, r) - c).max())
    print("%dx%d plane: error %.3g, numpy complex64 %.3g of the span; ratio %.2f"
          % (shape[0], shape[1], err / span, ref / span, err / ref))
    assert err <= RATIO * ref + FLOOR * span
    assert xl.shift_of_plane(got) == reg.calculate_shift(t, r)


def _plane_error(got, t, r, c):
    """(error, yardstick, span) of a GPU plane against the literal ``c``."""
    span = float(c.max() - c.min())
    err = float(np.abs(got - c).max())
    ref = float(np.abs(xl.plane_c64(t, r) - c).max())
    return err, ref, span


@pytest.mark.parametrize("case", ac.PLANE_CASES, ids=ac.case_id)
def test_plane_per_geometry(reg, case):
    """The whole plane, at every class of launch geometry reg_run can pick
    (align_cases.PLANE_CASES; test_align_cpu.py holds the table to the rule).
    No margin condition: the bound is on every value of the plane."""
    t, r = xl.blob_pair(case.shape, case.planted[0], case.planted[1], seed=7, dtype=case.dtype)
    c = xl.plane(t, r)
    got = reg.xcorr_plane(t, r)
    assert got.dtype == np.float32 and got.shape == case.shape
    err, ref, span = _plane_error(got, t, r, c)
    print("%dx%d %s plane (c = %d, %d groups): error %.3g, numpy complex64 %.3g of the span; "
          "ratio %.2f" % (case.shape[0], case.shape[1], np.dtype(case.dtype).name, case.c,
                          case.groups, err / span, ref / span, err / ref if ref else 0.0))
    assert err <= RATIO * ref + FLOOR * span, case.why
    assert xl.shift_of_plane(got) == reg.calculate_shift(t, r)
    _, _, peak = reg.calculate_shifts(t, r, return_peak=True)
    assert peak.dtype == np.float32 and peak[0].tobytes() == got.max().tobytes()


def _as_tensor(a):
    import torch
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda()


def test_batch_longer_than_a_chunk(reg):
    """7 full-size pairs where a launch holds 3: chunks of 3, 3 and 1 through
    one Z, one candidate table and the per-pair offsets into targets, sums,
    ref_of and results."""
    H, W = 2160, 2560
    L = hip.lib()
    assert ac.geometry(H, W, 7).chunk == 3
    assert 0 < L.tmh_register_scratch_bytes(7, 3, H, W) < 7 * H * W * 8
    targets, refs, ref_of, shifts = ac.rolled_batch((H, W))
    y, x, peak = reg.calculate_shifts(targets, refs, ref_of, return_peak=True)
    assert list(zip(y.tolist(), x.tolist())) == shifts
    singles = [reg.calculate_shifts(targets[i], refs[ref_of[i]], return_peak=True)
               for i in range(7)]
    assert [(int(s[0][0]), int(s[1][0])) for s in singles] == shifts
    assert np.array([s[2][0] for s in singles]).tobytes() == peak.tobytes()
    assert (peak > 0).all() and len(set(peak.tolist())) >= 3
    dy, dx, dpeak = reg.calculate_shifts(_as_tensor(targets), _as_tensor(refs), ref_of,
                                         return_peak=True)
    assert np.array_equal(dy, y) and np.array_equal(dx, x) and dpeak.tobytes() == peak.tobytes()


def test_more_pairs_than_one_launch_takes(reg):
    """32,769 pairs of 4x4: one more than a rows/cols launch and than a
    k_reg_sums launch takes, for targets and references alike."""
    targets, refs, ref_of, _ = ac.tiny_batch()
    n = len(targets)
    assert n == 32769 and ac.geometry(4, 4, n).chunk == 32768
    planes = ac.literal_planes(targets, refs, ref_of)
    want = ac.shifts_of_planes(planes)
    y, x, peak = reg.calculate_shifts(targets, refs, ref_of, return_peak=True)
    got = np.stack([y, x], axis=1)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, "%d pairs differ, the first is %d: gpu %s, literal %s" \
        % (bad.size, bad[0], got[bad[0]], want[bad[0]])
    # 200^2 * 15 / 16 in every pair; quarters and sixteenths of small integers are exact in f32
    lit = planes.reshape(n, -1).max(axis=1)
    assert np.array_equal(lit, np.full(n, 37500.0))
    bad = np.flatnonzero(peak != lit.astype(np.float32))
    assert bad.size == 0, "%d peaks differ, the first is %d: %r" % (bad.size, bad[0], peak[bad[0]])


def test_sums_beyond_one_launch(reg):
    """The sum of a target alone moves no plane that exact arithmetic can
    see: wrong by e, it adds e * sum(R - mean R) = 0, and at 4x4 every mean is
    a multiple of 1/16 and the f32 sum is zero as well.  At 3x5 the means are
    fifteenths, R - mean R is rounded, and its f32 sum is not zero.  So here
    one side of every pair is a constant image, whose plane is exactly 0.0
    when its own sum reaches it (Z is purely imaginary or purely real, and the
    single radix-3 and radix-5 passes keep its Hermitian halves bit for bit),
    and the other side has 15 random pixels.  Image 32,768, which the second
    k_reg_sums launch adds up, is the constant at the top of the type."""
    n = 32769
    assert ac.geometry(3, 5, n).chunk == 32768
    rng = np.random.default_rng(17)
    for dtype in (np.uint8, np.uint16):
        top = np.iinfo(dtype).max
        consts = np.empty((n, 3, 5), dtype)
        consts[:] = rng.integers(1, top + 1, n).astype(dtype)[:, None, None]
        consts[-1] = top
        noise = rng.integers(0, top + 1, (n, 3, 5)).astype(dtype)
        back = np.arange(n, dtype=np.int32)[::-1].copy()
        for name, targets, refs in (("constant targets", consts, noise),
                                    ("constant references", noise, consts)):
            for ref_of in (None, back):
                y, x, peak = reg.calculate_shifts(targets, refs, ref_of, return_peak=True)
                bad = np.flatnonzero((y != 0) | (x != 0) | (peak != 0.0))
                assert bad.size == 0, "%s, %s: %d pairs are not flat, the first is %d: (%d, %d), " \
                    "peak %r" % (np.dtype(dtype).name, name, bad.size, bad[0], y[bad[0]],
                                 x[bad[0]], peak[bad[0]])


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
@pytest.mark.parametrize("shape", [(37, 53), (1, 65)])
def test_sums_of_unaligned_images(reg, shape, dtype):
    """Images 1 and 2 of these stacks start off a 16-byte boundary, so
    k_reg_sums adds them up in its all-scalar loop.  A constant image minus its
    exact mean is exactly zero and so is every plane it takes part in: a sum
    that is off shows as a peak that is not 0.0."""
    px = shape[0] * shape[1]
    es = np.dtype(dtype).itemsize
    assert (px * es) % 16 != 0 and (2 * px * es) % 16 != 0
    top = np.iinfo(dtype).max
    consts = np.stack([np.full(shape, v, dtype) for v in (7, top, top // 2 + 1)])
    others = np.stack([np.full(shape, v, dtype) for v in (top - 1, 3, 100)])
    blobs = np.stack([xl.blob_pair(shape, 0, 0, seed=70 + k, dtype=dtype)[1] for k in range(3)])
    assert all(b.max() > b.min() for b in blobs)
    order = np.array([2, 0, 1], np.int32)
    for name, targets, refs in (("constant targets", consts, blobs),
                                ("constant references", blobs, consts),
                                ("constants", consts, others)):
        for ref_of in (None, order):
            y, x, peak = reg.calculate_shifts(targets, refs, ref_of, return_peak=True)
            print(name, y.tolist(), x.tolist(), peak.tolist())
            assert y.tolist() == [0, 0, 0] and x.tolist() == [0, 0, 0], name
            assert peak.tobytes() == np.zeros(3, np.float32).tobytes(), (name, peak.tolist())
    # blobs against blobs: each pair as in a call of its own, and at the literal's maximum
    shifts = [(2, -3), (0, 4), (-1, 1)] if shape[0] > 1 else [(0, -3), (0, 4), (0, 1)]
    targets = np.stack([xl.blob_pair(shape, dy, dx, seed=70 + int(k), dtype=dtype)[0]
                        for (dy, dx), k in zip(shifts, order)])
    y, x, peak = reg.calculate_shifts(targets, blobs, order, return_peak=True)
    for i in range(3):
        t, r = targets[i], blobs[order[i]]
        sy, sx, speak = reg.calculate_shifts(t, r, return_peak=True)
        assert (int(y[i]), int(x[i])) == (int(sy[0]), int(sx[0]))
        assert peak[i].tobytes() == speak[0].tobytes(), (i, peak[i], speak[0])
        c = xl.plane(t, r)
        _, ref, span = _plane_error(np.zeros(shape, np.float32), t, r, c)
        print("pair %d: peak %.9g, literal %.9g, yardstick %.3g" % (i, peak[i], c.max(), ref))
        assert abs(float(peak[i]) - float(c.max())) <= RATIO * ref + FLOOR * span


def test_device_entry_refusals(reg):
    """What tmh_register_shifts_device and tmh_xcorr_plane_device refuse on
    their own, each before any launch; the same buffers then register a pair."""
    L = hip.lib()
    H, W = 30, 40
    t, r = xl.blob_pair((H, W), 3, -5, seed=7)
    want, c = _checked_literal(t, r)
    sb = int(L.tmh_register_scratch_bytes(1, 1, H, W))
    assert sb > 0 and sb % 256 == 0
    rot = np.zeros(1, np.int32)
    y, x = np.full(1, 99, np.int32), np.full(1, 99, np.int32)
    peak = np.full(1, -1.0, np.float32)
    with hip.DeviceBuffer(t.nbytes + 2) as dt, hip.DeviceBuffer(r.nbytes + 2) as dr, \
            hip.DeviceBuffer(sb + 256) as scratch, hip.DeviceBuffer(4 * H * W + 4) as plane:
        assert scratch.value % 256 == 0 and plane.value % 4 == 0 and dt.value % 2 == 0
        dt.put(t)
        dr.put(r)
        plane.put(np.full((H, W), -7.0, np.float32))

        def shifts(tp=dt, rp=dr, sp=scratch, nbytes=sb):
            return L.tmh_register_shifts_device(tp, 1, rp, 1, H, W, 2, hip.ptr(rot), sp, nbytes,
                                                hip.ptr(y), hip.ptr(x), hip.ptr(peak), None)

        def xplane(tp=dt, rp=dr, sp=scratch, nbytes=sb, pp=plane):
            return L.tmh_xcorr_plane_device(tp, rp, H, W, 2, sp, nbytes, pp, None)

        for call in (shifts, xplane):
            for kwargs, words in (
                    (dict(sp=None), ("scratch", "NULL")),
                    (dict(sp=scratch.at(16, sb)), ("scratch", "aligned")),
                    (dict(nbytes=sb - 1), ("scratch", "smaller")),
                    (dict(tp=dt.at(1, t.nbytes)), ("images", "aligned")),
                    (dict(rp=dr.at(1, r.nbytes)), ("images", "aligned"))):
                rc = call(**kwargs)
                msg = L.tmh_last_error().decode()
                assert rc == hip.TMH_EINVAL, (call.__name__, kwargs, rc, msg)
                assert all(w in msg for w in words), (call.__name__, kwargs, msg)
        rc = xplane(pp=plane.at(2, 4 * H * W))
        msg = L.tmh_last_error().decode()
        assert rc == hip.TMH_EINVAL and "plane" in msg and "aligned" in msg, (rc, msg)
        # nothing ran: no result and no plane value was written
        assert (int(y[0]), int(x[0]), float(peak[0])) == (99, 99, -1.0)
        assert np.array_equal(plane.get((H, W), np.float32), np.full((H, W), -7.0, np.float32))
        hip.check(shifts())
        assert (int(y[0]), int(x[0])) == want
        hip.check(xplane())
        got = plane.get((H, W), np.float32)
        assert xl.shift_of_plane(got) == want and peak[0].tobytes() == got.max().tobytes()
        err, ref, span = _plane_error(got, t, r, c)
        assert err <= RATIO * ref + FLOOR * span


@pytest.mark.parametrize("dy,dx", [(6, 9), (6, -9), (-6, 9), (-6, -9)])
def test_round_trip_through_align(reg, dy, dx):
    """Shifts [0, (dy, dx)] -> residues -> metadata -> Image.align(crop=True):
    a noise-free pair with T[r, c] = R[r + dy, c + dx] comes out equal, which
    ties the sign and the residue assignment to the golden-pinned align."""
    from tmlibrary_amd.image import ChannelImage
    from tmlibrary_amd.metadata import ChannelImageMetadata
    from tmlibrary_amd.workflow.align import api as align_api
    t, r = xl.blob_pair((120, 160), dy, dx, seed=21, noise=False)
    assert np.array_equal(t[20:90, 20:100], r[20 + dy:90 + dy, 20 + dx:100 + dx])
    _checked_literal(t, r)
    result = align_api.AlignmentResult()
    shifts = [reg.calculate_shift(r, r), reg.calculate_shift(t, r)]
    assert shifts == [(0, 0), (dy, dx)]
    for cycle, s in enumerate(shifts):
        result.shifts[(1, cycle)] = s
    result.residues[1] = align_api.site_residues([s[0] for s in shifts], [s[1] for s in shifts])
    out = []
    for cycle, img in enumerate((r, t)):
        md = align_api.fill_metadata(ChannelImageMetadata(0, 1, cycle, 0, 0), result)
        aligned = ChannelImage(img.copy(), md).align(crop=True).array
        res = result.residues[1]
        want = orc.shift_and_crop(img, md.y_shift, md.x_shift, res["bottom"], res["top"],
                                  res["right"], res["left"], crop=True)
        assert np.array_equal(aligned, want)
        out.append(aligned)
    assert out[0].shape == (120 - abs(dy), 160 - abs(dx))
    assert np.array_equal(out[0], out[1])


def _two_cycle_store(tmp_path, shifts, planes=None):
    """4 sites x 2 cycles of 96 x 128 gzip-HDF5 files (h5py's chunking), cycle
    1 shifted against cycle 0 by ``shifts``; optional per-channel statistics."""
    from tmlibrary_amd.models.file import ExperimentStore, write_channel_image, write_illumstats
    os.makedirs(str(tmp_path / "channel_image_files"))
    info, cycle_files, images = {}, [(0, {}), (1, {})], {}
    for site, (dy, dx) in enumerate(shifts):
        t, r = xl.blob_pair((96, 128), dy, dx, seed=60 + site)
        for cycle, img in ((0, r), (1, t)):
            fid = 100 * cycle + site
            info[fid] = (cycle, site, cycle, 0, 0)  # channel = cycle: own statistics per cycle
            cycle_files[cycle][1][site] = [fid]
            images[fid] = img
    store = ExperimentStore(str(tmp_path), file_info=info)
    for fid, img in images.items():
        write_channel_image(store.channel_image_file(fid).location, img, gzip_level=4)
    if planes is not None:
        for channel, (mean, std) in planes.items():
            write_illumstats(store.illumstats_file(channel).location, mean, std, {50.0: 300})
    return store, cycle_files, images


def _stat_planes():
    yy, xx = np.mgrid[0:96, 0:128]
    out = {}
    for channel in (0, 1):
        mean = 2.45 + 0.1 * channel + 0.15 * np.exp(-((yy - 48) ** 2 + (xx - 64) ** 2) / 6000.0)
        std = 0.22 + 0.03 * (xx / 128.0) + 0.02 * channel
        out[channel] = (mean, std)
    return out


@pytest.mark.parametrize("illumcorr", [False, True])
@pytest.mark.parametrize("decode", ["auto", "host"])
def test_run_job(reg, tmp_path, illumcorr, decode):
    from tmlibrary_amd.models.file import h5lib
    from tmlibrary_amd.workflow.align import api as align_api
    h5lib()
    shifts = [(3, -5), (-7, 2), (0, 0), (8, 11)]
    planes = _stat_planes()
    store, cycle_files, images = _two_cycle_store(tmp_path, shifts, planes)
    registrator = align_api.ImageRegistrator(1, store=store, block=3, decode=decode)
    args = align_api.AlignBatchArguments(ref_cycle=0, ref_wavelength="DAPI", batch_size=100,
                                         illumcorr=illumcorr)
    batches = list(registrator.create_run_batches(args, cycle_files=cycle_files))
    assert len(batches) == 1
    result = registrator.run_job(batches[0])
    assert registrator.last_path == ("gpu" if decode == "auto" else "host")

    def corrected(fid):
        img = images[fid]
        if not illumcorr:
            return img
        mean, std = planes[fid // 100]
        return orc.correct_illumination(img, orc.smooth_reflect(mean), orc.smooth_reflect(std))

    for site in range(4):
        ref = corrected(site)
        ys, xs = [], []
        for cycle in (0, 1):
            # the oracle's plane must hold the condition with room for the +-1 DN
            # the GPU correction may differ by
            want, _ = _checked_literal(corrected(100 * cycle + site), ref)
            assert result.shifts[(site, cycle)] == want, (site, cycle)
            ys.append(want[0])
            xs.append(want[1])
        assert result.shifts[(site, 0)] == (0, 0)
        assert result.residues[site] == align_api.site_residues(ys, xs)
    assert store.site_shifts == result.shifts and store.site_residues == result.residues


def test_errors(reg):
    a = np.zeros((30, 40), np.uint16)
    with pytest.raises(ValueError, match="differ in shape"):
        reg.calculate_shift(a, np.zeros((30, 41), np.uint16))
    with pytest.raises(ValueError, match="4096"):
        reg.calculate_shift(np.zeros((2, 4097), np.uint16), np.zeros((2, 4097), np.uint16))
    with pytest.raises(ValueError, match="4096"):  # 2053 is prime: padded to >= 4105
        reg.calculate_shift(np.zeros((2, 2053), np.uint8), np.zeros((2, 2053), np.uint8))
    with pytest.raises(ValueError, match="outside the references"):
        reg.calculate_shifts(np.stack([a, a]), a[None], np.array([0, 1], np.int32))
    with pytest.raises(TypeError):
        reg.calculate_shift(a.astype(np.float32), a.astype(np.float32))


@pytest.mark.parametrize("L", [4096, 2047])
def test_longest_lines(reg, L):
    """The limits themselves are valid, as rows and as columns: a 5-smooth
    4096, and 2047 = 23 * 89, padded to 4093 -> 4096."""
    wide = np.zeros((1, L), np.uint16)
    wide[0, 7] = 1000
    wide[0, 100] = 300
    assert reg.calculate_shift(np.roll(wide, -3, axis=1), wide) == (0, 3)
    assert reg.calculate_shift(np.roll(wide, 5, axis=1), wide) == (0, -5)
    tall = np.ascontiguousarray(wide.T)
    assert reg.calculate_shift(np.roll(tall, -3, axis=0), tall) == (3, 0)
    both = np.zeros((3, L), np.uint16)
    both[1, 7], both[2, 100] = 1000, 300
    assert reg.calculate_shift(np.roll(both, (-1, 4), axis=(0, 1)), both) == (1, -4)
