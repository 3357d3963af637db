"""CPU: the align step's rules and the line FFT's arithmetic, without a GPU.

* ``calculate_overlap`` against goldens computed by the reference
  (tests/golden/make_align_goldens.py) and the literal residue assignment;
* the numpy literal of the correlation (tests/xcorr_literal.py) against the
  direct sum;
* tests/align_cases.py: the launch geometry of every plane case the GPU tests
  run, the classes the table must cover, and the batches' planted shifts
  under the literal;
* the job dicts and errors of ``ImageRegistrator.create_run_batches``;
* tmlibrary_amd/csrc/fft_core.h -- the exact per-line code the registration
  kernels run -- compiled with g++ (tests/fft_host.cpp) and compared with
  numpy.  The bound: numpy's own complex64 transform against numpy's f64
  transform is the yardstick for what single precision costs; the harness may
  miss the f64 result by 4x that plus 1e-7 of the largest magnitude.  The
  margin is for another radix order and twiddle rounding, not for a wrong
  algorithm, which misses by orders of magnitude.
"""
import os
import subprocess

import numpy as np
import pytest

import align_cases as ac
import xcorr_literal as xl
from util import REPO, load_golden
from tmlibrary_amd.metadata import ChannelImageMetadata
from tmlibrary_amd.models.file import ExperimentStore
from tmlibrary_amd.workflow.align import api as align_api
from tmlibrary_amd.workflow.align import registration as reg

HARNESS = os.path.join(REPO, "tests", "fft_host.cpp")
FLAGS = ["-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas"]
LINE_LENGTHS = (1, 2, 3, 5, 8, 9, 25, 30, 48, 81, 125, 270, 2160, 2560)
PADDED_LENGTHS = (37, 53)
RATIO, FLOOR = 4.0, 1e-7


# ---- overlap and residues ------------------------------------------------------------
def test_overlap_equals_reference_goldens():
    g = load_golden("align_overlap")
    n = int(g["n_cases"])
    assert n >= 20
    for i in range(n):
        ys, xs = g["y_%02d" % i].tolist(), g["x_%02d" % i].tolist()
        got = reg.calculate_overlap(ys, xs)
        assert list(got) == g["overlap_%02d" % i].tolist(), (ys, xs)
        assert all(isinstance(v, int) for v in got)


def test_overlap_rule():
    assert reg.calculate_overlap([0, 4, -7], [0, -2, 9]) == (7, 4, 9, 2)  # top, bottom, right, left
    assert reg.calculate_overlap([], []) == (0, 0, 0, 0)


def test_residue_assignment_is_the_references():
    """run_job unpacks (top, bottom, right, left) as bottom, top, left, right:
    top receives the largest positive y shift, left the largest positive x."""
    res = align_api.site_residues([0, 4, -7], [0, -2, 9])
    assert res == {"top": 4, "bottom": 7, "left": 9, "right": 2}
    # so _shift_and_crop's row_start = top - y and col_start = left - x stay >= 0
    for y, x in ((0, 0), (4, -2), (-7, 9)):
        assert res["top"] - y >= 0 and res["left"] - x >= 0


def test_fill_metadata():
    result = align_api.AlignmentResult()
    result.shifts[(5, 1)] = (3, -2)
    result.residues[5] = {"top": 3, "bottom": 0, "left": 0, "right": 2}
    md = align_api.fill_metadata(ChannelImageMetadata(0, 5, 1, 0, 0), result)
    assert (md.y_shift, md.x_shift) == (3, -2)
    assert (md.top_residue, md.bottom_residue, md.left_residue, md.right_residue) == (3, 0, 0, 2)
    with pytest.raises(KeyError):
        align_api.fill_metadata(ChannelImageMetadata(0, 6, 1, 0, 0), result)


# ---- the literal ---------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1), (1, 7), (6, 1), (5, 8), (12, 12), (9, 10)])
def test_literal_equals_direct_sum(shape):
    rng = np.random.default_rng(shape[0] * 100 + shape[1])
    t = rng.integers(0, 4000, shape).astype(np.uint16)
    r = rng.integers(0, 4000, shape).astype(np.uint16)
    want = xl.brute_plane(t, r)
    got = xl.plane(t, r)
    assert np.abs(got - want).max() <= 1e-9 * max(1.0, np.abs(want).max())


def test_literal_sign_and_mapping():
    rng = np.random.default_rng(5)
    r = rng.integers(0, 4000, (10, 12)).astype(np.uint16)
    for dy, dx in ((2, -3), (-4, 5), (0, 0), (5, 6), (-4, -5)):
        t = np.roll(r, (-dy, -dx), axis=(0, 1))  # T[r, c] = R[r + dy, c + dx], cyclic
        assert xl.shift(t, r) == (dy, dx)
        assert xl.shift_of_plane(xl.brute_plane(t, r)) == (dy, dx)
    # a lag of exactly L / 2 stays positive; beyond it the lag is negative
    assert [xl.signed_lag(d, 10) for d in (0, 5, 6, 9)] == [0, 5, -4, -1]
    assert [xl.signed_lag(d, 7) for d in (3, 4)] == [3, -3]
    # ties: the lowest flat unsigned lag; two constant images are one big tie
    assert xl.shift(np.full((4, 6), 9, np.uint16), np.full((4, 6), 70, np.uint16)) == (0, 0)
    assert xl.shift_of_plane(np.array([[1.0, 3.0, 3.0], [3.0, 0.0, 3.0]])) == (0, 1)


# ---- the GPU tests' case table and batches (tests/align_cases.py) --------------------
@pytest.mark.parametrize("case", ac.PLANE_CASES, ids=ac.case_id)
def test_plane_case_is_what_the_table_says(case):
    """The launch geometry is the table's, and the complex64 yardstick of the
    plane bound is positive (2x2 is exact in both precisions)."""
    H, W = case.shape
    g = ac.geometry(H, W)
    assert (g.Mh, g.Mw, g.c, g.half_cols, g.groups) == \
        (case.Mh, case.Mw, case.c, case.half_cols, case.groups), case.why
    assert g.stride == g.Mh | 1 and g.chunk == 1
    assert 4 * g.c * g.stride * 8 <= ac.LDS_BYTES
    t, r = xl.blob_pair(case.shape, case.planted[0], case.planted[1], seed=7, dtype=case.dtype)
    c = xl.plane(t, r)
    assert c.max() > c.min()
    ref = float(np.abs(xl.plane_c64(t, r) - c).max())
    if case.shape == (2, 2):
        assert ref == 0.0
    else:
        assert ref > 0.0


def test_plane_cases_cover_every_class():
    cases = ac.PLANE_CASES
    assert len({c.shape for c in cases}) == len(cases) >= 18
    assert {c.c for c in cases} == {1, 2, 4, 7, 8}
    assert any(c.c == c.half_cols < 8 and c.c > 1 for c in cases)
    assert {c.Mw % 2 for c in cases} == {0, 1}
    assert any(c.Mw % 2 == 1 and c.Mw == c.shape[1] > 1 for c in cases)   # odd, unpadded
    assert any(c.Mw % 2 == 1 and c.Mw > c.shape[1] for c in cases)        # padded to odd
    assert {(c.Mh > c.shape[0], c.Mw > c.shape[1]) for c in cases} == \
        {(False, False), (False, True), (True, False), (True, True)}
    assert any(1 < c.groups < 8 for c in cases)
    assert any(c.groups > 8 and c.groups % 8 for c in cases)
    assert any(c.groups * c.c > c.half_cols for c in cases)                # padding slots
    assert any(c.shape[0] == 1 for c in cases) and any(c.shape[1] == 1 for c in cases)
    assert any(c.shape[1] > 256 for c in cases)
    u8 = [c for c in cases if c.dtype == np.uint8]
    assert len(u8) >= 4
    assert any(max(c.shape) <= 64 for c in u8)                             # small
    assert any((c.Mh, c.Mw) != c.shape for c in u8)                        # padded
    assert any(c.shape[0] > 700 for c in u8)                               # tall


def test_rolled_batch_gives_its_rolls():
    """The 7-pair batch at a small shape, every pair under the literal; at
    full size one pair (the others hold by the same construction)."""
    targets, refs, ref_of, shifts = ac.rolled_batch((54, 64))
    assert len(set(shifts)) == 7 and (0, 0) in shifts
    assert any(dy < 0 for dy, _ in shifts) and any(dx < 0 for _, dx in shifts)
    assert sorted(set(ref_of.tolist())) == [0, 1, 2]
    planes = ac.literal_planes(targets, refs, ref_of)
    for i in range(7):
        assert np.allclose(planes[i], xl.plane(targets[i], refs[ref_of[i]]), rtol=0, atol=1e-6)
        assert xl.peak_margin(planes[i]) > 0.5
    assert ac.shifts_of_planes(planes).tolist() == [list(s) for s in shifts]
    targets, refs, ref_of, shifts = ac.rolled_batch((2160, 2560))
    assert targets.dtype == np.uint8 and targets.shape == (7, 2160, 2560)
    assert all(np.count_nonzero(r) >= 38 for r in refs)
    i = 4                                                                  # (-1, -12)
    c = xl.plane(targets[i], refs[ref_of[i]])
    assert xl.shift_of_plane(c) == shifts[i] and xl.peak_margin(c) > 0.5
    for j in range(7):
        assert np.array_equal(np.roll(targets[j], shifts[j], axis=(0, 1)), refs[ref_of[j]])


def test_tiny_batch_gives_its_shifts():
    """One pair more than a launch takes: the literal recovers every planted
    shift, and each peak stands a whole span above the rest of its plane."""
    targets, refs, ref_of, shifts = ac.tiny_batch()
    n = len(targets)
    assert n == len(refs) == ac.MAX_LAUNCH + 1 and ac.geometry(4, 4, n).chunk == ac.MAX_LAUNCH
    assert sorted(ref_of.tolist()) == list(range(n)) and not np.array_equal(ref_of, np.arange(n))
    assert {tuple(s) for s in shifts.tolist()} == {(a, b) for a in range(-1, 3) for b in range(-1, 3)}
    planes = ac.literal_planes(targets, refs, ref_of)
    got = ac.shifts_of_planes(planes)
    bad = np.flatnonzero((got != shifts).any(axis=1))
    assert bad.size == 0, "pair %d: literal %s, planted %s" % (bad[0], got[bad[0]], shifts[bad[0]])
    flat = np.sort(planes.reshape(n, -1), axis=1)
    margin = (flat[:, -1] - flat[:, -2]) / (flat[:, -1] - flat[:, 0])
    assert np.abs(margin - 1.0).max() < 1e-12


# ---- jobs ----------------------------------------------------------------------------
def _registrator(tmp_path):
    return align_api.ImageRegistrator(1, store=ExperimentStore(str(tmp_path)))


def test_batch_dicts(tmp_path):
    cycle_files = [(10, {1: [101], 2: [102], 3: [103]}), (11, {1: [111], 2: [112], 3: [113]})]
    args = align_api.AlignBatchArguments(ref_cycle=1, ref_wavelength="DAPI", batch_size=2,
                                         illumcorr=True)
    batches = list(_registrator(tmp_path).create_run_batches(args, cycle_files=cycle_files))
    assert [b["id"] for b in batches] == [1, 2]
    for b in batches:
        assert sorted(b) == ["id", "illumcorr", "input_ids"]
        assert sorted(b["input_ids"]) == ["reference_file_ids", "target_file_ids"]
        assert b["illumcorr"] is True
    assert batches[0]["input_ids"]["reference_file_ids"] == [111, 112]
    assert dict(batches[0]["input_ids"]["target_file_ids"]) == {10: [101, 102], 11: [111, 112]}
    assert batches[1]["input_ids"]["reference_file_ids"] == [113]
    assert dict(batches[1]["input_ids"]["target_file_ids"]) == {10: [103], 11: [113]}


def test_batch_errors(tmp_path):
    r = _registrator(tmp_path)
    args = align_api.AlignBatchArguments(ref_cycle=0, ref_wavelength="DAPI")
    with pytest.raises(align_api.NotSupportedError, match="more than one cycle"):
        list(r.create_run_batches(args, cycle_files=[(10, {1: [101]})]))
    two = [(10, {1: [101]}), (11, {1: [111]})]
    args.ref_cycle = 2
    with pytest.raises(align_api.JobDescriptionError, match="must not exceed"):
        list(r.create_run_batches(args, cycle_files=two))
    args.ref_cycle = 0
    with pytest.raises(ValueError, match="No image files found for cycle 11"):
        list(r.create_run_batches(args, cycle_files=[(10, {1: [101]}), (11, {})]))
    with pytest.raises(ValueError):
        align_api.ImageRegistrator(1)
    with pytest.raises(TypeError):
        align_api.ImageRegistrator(1, store=object())


# ---- the line FFT --------------------------------------------------------------------
def _build(out, extra=()):
    return subprocess.run(["g++", "-O2"] + list(extra) + FLAGS + ["-o", out, HARNESS],
                          capture_output=True, text=True)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("fft") / "fft_host")
    r = _build(out)
    assert r.returncode == 0, r.stderr
    return out


def _line(L):
    rng = np.random.default_rng(1000 + L)
    return (rng.normal(size=L) + 1j * rng.normal(size=L)).astype(np.complex64)


def _run_fft(exe, tmp_path, z):
    p = lambda name: str(tmp_path / name)  # noqa: E731
    z.tofile(p("in"))
    subprocess.run([exe, "fft", str(len(z)), p("in"), p("out")], check=True)
    out = np.fromfile(p("out"), np.complex64)
    assert out.size == 2 * len(z)
    return out[:len(z)], out[len(z):]


def _run_corr(exe, tmp_path, a, b):
    p = lambda name: str(tmp_path / name)  # noqa: E731
    np.concatenate([a, b]).astype(np.float32).tofile(p("cin"))
    subprocess.run([exe, "corr", str(len(a)), p("cin"), p("cout")], check=True)
    out = np.fromfile(p("cout"), np.float32)
    assert out.size == len(a)
    return out


def _check_fft(exe, tmp_path, L):
    """-> (forward ratio, round-trip ratio) of the harness's error to numpy's
    complex64 error, after asserting the bound."""
    z = _line(L)
    fwd, back = _run_fft(exe, tmp_path, z)
    z64 = z.astype(np.complex128)
    want = np.fft.fft(z64)
    np32 = np.fft.fft(z)
    assert np32.dtype == np.complex64, "numpy promoted the single-precision transform"
    err, ref = np.abs(fwd - want).max(), np.abs(np32 - want).max()
    mag = np.abs(want).max()
    print("L=%d forward: error %.3g, numpy complex64 %.3g, of max %.3g" % (L, err, ref, mag))
    assert err <= RATIO * ref + FLOOR * mag, (L, err, ref)
    # the inverse, on the harness's own forward result: against numpy f64 of that input
    want_b = np.fft.ifft(fwd.astype(np.complex128)) * L
    np32_b = np.fft.ifft(fwd) * np.float32(L)
    err_b, ref_b = np.abs(back - want_b).max(), np.abs(np32_b - want_b).max()
    mag_b = np.abs(want_b).max()
    print("L=%d inverse: error %.3g, numpy complex64 %.3g, of max %.3g" % (L, err_b, ref_b, mag_b))
    assert err_b <= RATIO * ref_b + FLOOR * mag_b, (L, err_b, ref_b)
    return err / max(ref, 1e-300), err_b / max(ref_b, 1e-300)


def _check_corr(exe, tmp_path, L):
    rng = np.random.default_rng(2000 + L)
    a = rng.normal(size=L).astype(np.float32)
    b = rng.normal(size=L).astype(np.float32)
    got = _run_corr(exe, tmp_path, a, b)
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    want = np.array([np.sum(a64 * np.roll(b64, -d)) for d in range(L)])  # the definition
    np32 = np.fft.ifft(np.conj(np.fft.fft(a.astype(np.complex64))) *
                       np.fft.fft(b.astype(np.complex64))).real
    err, ref = np.abs(got - want).max(), np.abs(np32 - want).max()
    mag = np.abs(want).max()
    print("L=%d correlation: error %.3g, numpy complex64 %.3g, of max %.3g" % (L, err, ref, mag))
    assert err <= RATIO * ref + FLOOR * mag, (L, err, ref)


@pytest.mark.parametrize("L", LINE_LENGTHS)
def test_line_transform_against_numpy(exe, tmp_path, L):
    _check_fft(exe, tmp_path, L)


@pytest.mark.parametrize("L", PADDED_LENGTHS + (30, 64))
def test_pad_and_fold_correlation(exe, tmp_path, L):
    """Lengths with a prime factor above 5 go through the zero-padded linear
    correlation and the fold back to period L (30 and 64: the plain path)."""
    _check_corr(exe, tmp_path, L)


def test_harness_rejects_a_rough_length(exe, tmp_path):
    z = _line(37)
    z.tofile(str(tmp_path / "in"))
    r = subprocess.run([exe, "fft", "37", str(tmp_path / "in"), str(tmp_path / "out")])
    assert r.returncode == 4  # 37 is no 5-smooth length: no plan


def test_line_transform_under_sanitizers(tmp_path):
    """The same harness with -fsanitize=address,undefined: every line, table
    and scratch is a heap block of its exact size."""
    exe = str(tmp_path / "fft_host_san")
    r = _build(exe, ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    if r.returncode != 0 and ("asan" in r.stderr or "ubsan" in r.stderr or "sanitize" in r.stderr):
        pytest.skip("g++ here lacks the sanitizer runtimes: " + r.stderr.strip().splitlines()[-1])
    assert r.returncode == 0, r.stderr
    for L in LINE_LENGTHS:
        _check_fft(exe, tmp_path, L)
    for L in PADDED_LENGTHS:
        _check_corr(exe, tmp_path, L)
