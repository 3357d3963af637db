"""GPU: what a host-buffer entry point reports when the failure (or the
behaviour) comes from the body it shares with its ``_device`` form, after the
wrapper has staged its buffers: the error code and the message text, the
measuring call of the JPEG encoder, the line-limit error of an empty
registration call, and the destination bytes an odd mosaic keeps."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
T = 256


@pytest.fixture(scope="module")
def L():
    from tmlibrary_amd import hip
    return hip.lib()


def _fails(L, rc):
    """(code, message) of a failed call."""
    assert rc != 0
    return rc, L.tmh_last_error().decode()


@pytest.fixture(scope="module")
def chain(L):
    """One 16 x 16 site, its corrector and a whole-image window."""
    from tmlibrary_amd import hip
    rng = np.random.default_rng(5)
    mean = rng.uniform(2.0, 3.0, (16, 16))
    std = rng.uniform(0.1, 0.2, (16, 16))
    c = C.c_void_p()
    hip.check(L.tmh_corrector_create(hip.ptr(mean), hip.ptr(std), 16, 16, 1, -10.0, C.byref(c)))
    site = rng.integers(100, 4000, (1, 16, 16), dtype=np.uint16)
    win = np.zeros(1, dtype=hip.WINDOW_DTYPE)
    win["rows"], win["cols"] = 16, 16
    yield c, site, win
    L.tmh_corrector_destroy(c)


def test_chain_scale_error_comes_from_the_shared_body(L, chain):
    from tmlibrary_amd import hip
    c, site, win = chain
    out = np.zeros((1, 16, 16), dtype=np.uint8)
    rc, msg = _fails(L, L.tmh_correct_chain_u8(c, hip.ptr(site), hip.ptr(out), 1, hip.ptr(win),
                                               300, 300))
    assert rc == hip.TMH_EINVAL
    assert msg == '"lower_bound" must be smaller than "upper_bound"'


def test_chain_window_error_comes_from_the_shared_body(L, chain):
    from tmlibrary_amd import hip
    c, site, win = chain
    bad = win.copy()
    bad["src_r0"] = 8          # rows 8 .. 24 of a 16-row site
    out = np.zeros((1, 16, 16), dtype=np.uint8)
    rc, msg = _fails(L, L.tmh_correct_chain_u8(c, hip.ptr(site), hip.ptr(out), 1, hip.ptr(bad),
                                               100, 4000))
    assert rc == hip.TMH_EINVAL
    assert msg == "alignment window leaves the source image"
    # the same call with the good window goes through
    hip.check(L.tmh_correct_chain_u8(c, hip.ptr(site), hip.ptr(out), 1, hip.ptr(win), 100, 4000))


def test_jpeg_encode_measures_then_checks_the_capacity(L):
    from tmlibrary_amd import hip
    level = np.random.default_rng(6).integers(0, 256, (1, T, T), dtype=np.uint8)
    offsets, total = np.full(2, -1, dtype=np.int64), C.c_int64(0)
    rc = L.tmh_jpeg_encode_level(hip.ptr(level), 1, 1, T, T, 95, None, 0, hip.ptr(offsets),
                                 C.byref(total))
    assert rc == hip.TMH_OK and total.value > 0
    assert offsets.tolist() == [0, total.value]
    n = total.value
    out = np.zeros(n, dtype=np.uint8)
    rc, msg = _fails(L, L.tmh_jpeg_encode_level(hip.ptr(level), 1, 1, T, T, 95, hip.ptr(out), n - 1,
                                                hip.ptr(offsets), C.byref(total)))
    assert rc == hip.TMH_EINVAL
    assert msg == "the output holds %d bytes, the level's files %d" % (n - 1, n)
    assert not out.any(), "nothing is written into an output that is too small"


def test_register_without_targets_still_reports_the_line_limit(L):
    from tmlibrary_amd import hip
    rc, msg = _fails(L, L.tmh_register_shifts(None, 0, None, 0, 16, 5000, 2, None, None, None, None))
    assert rc == hip.TMH_EINVAL
    assert msg == "an image side is over the limit of 4096 values"
    assert L.tmh_register_shifts(None, 0, None, 0, 16, 16, 2, None, None, None, None) == hip.TMH_OK


def test_shrink_returns_an_odd_mosaics_tile_as_passed_in(L):
    from tmlibrary_amd import hip
    rng = np.random.default_rng(7)
    level = rng.integers(0, 256, (1, 1, T, T), dtype=np.uint8)
    dst = rng.integers(0, 256, (1, 1, T, T), dtype=np.uint8)
    keep = dst.copy()
    oh, ow = C.c_int(-1), C.c_int(-1)
    hip.check(L.tmh_pyramid_shrink2(hip.ptr(level), 1, 1, 255, T, hip.ptr(dst), C.byref(oh),
                                    C.byref(ow)))
    assert (oh.value, ow.value) == (127, 128)
    assert np.array_equal(dst, keep)


def test_retired_option_values_are_refused(L):
    """Option values whose code paths were removed (fused configurations 0, 1,
    2 and 4; option 5, the host staging mode) are TMH_EINVAL, the remaining
    ones are accepted and reported back; the option calls launch no kernel."""
    from tmlibrary_amd import hip
    from tmlibrary_amd.workflow.corilla.quantiles import quantile_table, stats_log10_lut
    H = W = 32
    lo, hi, gamma = quantile_table(H * W, np.linspace(0, 100, 1000))
    lut = stats_log10_lut()
    h = C.c_void_p()
    hip.check(L.tmh_stats_create(H, W, 1000, hip.ptr(lo), hip.ptr(hi), hip.ptr(gamma),
                                 hip.ptr(lut), 1, 0, C.byref(h)))
    c = C.c_void_p()
    mean, std = np.full((H, W), 2.5), np.full((H, W), 0.15)
    hip.check(L.tmh_corrector_create(hip.ptr(mean), hip.ptr(std), H, W, 1, -10.0, C.byref(c)))
    try:
        for v in (0, 1, 2, 4, 6, -2):
            rc, msg = _fails(L, L.tmh_stats_set_option(h, hip.TMH_OPT_FUSED_CONFIG, v))
            assert rc == hip.TMH_EINVAL, v
            assert ("retired" in msg) == (v in (0, 1, 2, 4)), (v, msg)
        fc = C.c_int(-7)
        for v in (-1, 3, 5, 100):
            assert L.tmh_stats_set_option(h, hip.TMH_OPT_FUSED_CONFIG, v) == hip.TMH_OK, v
            hip.check(L.tmh_stats_job_choice(h, None, None, C.byref(fc)))
            assert fc.value == (3 if v == -1 else v), (v, fc.value)  # unprobed: narrow
        assert hip.TMH_FUSED_NO_HIST == 100
        for set_option, handle in ((L.tmh_stats_set_option, h), (L.tmh_corrector_set_option, c)):
            rc, msg = _fails(L, set_option(handle, 5, 2))
            assert rc == hip.TMH_EINVAL and "unknown" in msg, msg
            for v in (1, 64):
                assert set_option(handle, hip.TMH_OPT_COPY_THREADS, v) == hip.TMH_OK, v
            for v in (0, 65):
                rc, msg = _fails(L, set_option(handle, hip.TMH_OPT_COPY_THREADS, v))
                assert rc == hip.TMH_EINVAL and msg == "copy threads must be 1..64", (v, msg)
    finally:
        L.tmh_corrector_destroy(c)
        L.tmh_stats_destroy(h)
