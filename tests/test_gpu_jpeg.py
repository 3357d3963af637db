"""GPU: JPEG coding of pyramid tiles through the C-ABI (k_jpeg_tiles) and the
Python layer (``Pyramid.encode_level`` / ``iter_jpeg_tiles``,
``PyramidTile.jpeg_encode``).  Everything is byte-exact: against the files
libjpeg-turbo wrote (tests/golden/jpeg_tiles.npz; no test here imports
Pillow) and against tests/jpeg_literal.py, which the CPU suite pins to them.
"""
import contextlib
import ctypes as C
import hashlib
import os

import numpy as np
import pytest

import jpeg_literal as jl
import pyramid_literal as lit
from tmlibrary_amd import hip
from util import REPO

pytestmark = pytest.mark.gpu
T = 256
GUARD = 64


@pytest.fixture(scope="module")
def L():
    return hip.lib()


@pytest.fixture(scope="module")
def goldens():
    return jl.load_goldens(os.path.join(REPO, "tests", "golden", "jpeg_tiles.npz"))


@pytest.fixture(scope="module")
def literal():
    """jpeg_literal.encode, each distinct (array, quality) coded once."""
    cache = {}

    def get(a, q=95):
        key = (a.shape, q, hashlib.sha1(np.ascontiguousarray(a)).digest())
        if key not in cache:
            cache[key] = jl.encode(a, q)
        return cache[key]
    return get


def _level(tiles, rows, cols, surround=0):
    """[rows][cols][256][256] storage with tile t's array in its corner and
    ``surround`` in the rest of a ragged tile's storage."""
    level = np.full((rows * cols, T, T), surround, dtype=np.uint8)
    for t, a in enumerate(tiles):
        level[t, :a.shape[0], :a.shape[1]] = a
    return level


def _encode(L, level, rows, cols, last_h, last_w, quality, write=True):
    """One writing (or measuring) call -> (rc, blob incl. guard, offsets, total)."""
    n = rows * cols
    total = C.c_int64(-1)
    with contextlib.ExitStack() as stack:
        d_level = stack.enter_context(hip.DeviceBuffer.from_array(level))
        d_off = stack.enter_context(hip.DeviceBuffer.from_array(np.full(n + 1, -1, dtype=np.int64)))
        rc = L.tmh_jpeg_encode_level_device(d_level, rows, cols, last_h, last_w, quality, None, 0,
                                            d_off, C.byref(total), None)
        assert rc == 0, L.tmh_last_error()
        measured = d_off.get(n + 1, np.int64)
        assert total.value == measured[n] and measured[0] == 0
        if not write:
            return rc, None, measured, total.value
        d_out = stack.enter_context(hip.DeviceBuffer.from_array(
            np.full(total.value + GUARD, 0x5C, dtype=np.uint8)))
        total2 = C.c_int64(-1)
        rc = L.tmh_jpeg_encode_level_device(d_level, rows, cols, last_h, last_w, quality, d_out,
                                            total.value, d_off, C.byref(total2), None)
        assert rc == 0, L.tmh_last_error()
        offsets = d_off.get(n + 1, np.int64)
        # the measuring call and the writing call agree
        assert total2.value == total.value and np.array_equal(offsets, measured)
        return rc, d_out.get(total.value + GUARD, np.uint8), offsets, total.value


def _files(blob, offsets):
    return [blob[offsets[t]:offsets[t + 1]].tobytes() for t in range(len(offsets) - 1)]


# ---- goldens, one tile at a time -----------------------------------------------------

@pytest.mark.parametrize("case", [c[0] for c in jl.GOLDEN_CASES])
def test_golden_as_a_one_tile_level(L, goldens, case):
    name, a, q, want = [g for g in goldens if g[0] == case][0]
    h, w = a.shape
    _, blob, offsets, total = _encode(L, _level([a], 1, 1, surround=0xAA), 1, 1, h, w, q)
    assert total == len(want) and offsets.tolist() == [0, len(want)]
    assert blob[:total].tobytes() == want
    assert np.all(blob[total:] == 0x5C)


# ---- one mixed level ---------------------------------------------------------------------

KINDS = ("zeros", "noise", "stripes", "cells", "full", "checker8", "specks", "smooth", "checker1",
         "impulses", "ramp")


def test_mixed_ragged_level(L, literal):
    """5 x 7 tiles, last row 37 high, last column 101 wide, the kinds cycling
    so that neighbouring files differ in size from 1,100 to tens of thousands
    of bytes; 0xAA around the ragged tiles."""
    rows, cols, lh, lw = 5, 7, 37, 101
    tiles = []
    for t in range(rows * cols):
        y, x = divmod(t, cols)
        shape = (lh if y == rows - 1 else T, lw if x == cols - 1 else T)
        tiles.append(jl.case_array(KINDS[t % len(KINDS)], shape))
    _, blob, offsets, total = _encode(L, _level(tiles, rows, cols, surround=0xAA), rows, cols, lh,
                                      lw, 95)
    want = [literal(a) for a in tiles]
    sizes = np.diff(offsets)
    assert np.all(sizes > 0), "offsets must be strictly increasing"
    assert sizes.tolist() == [len(w) for w in want]
    assert sizes.min() <= 1100 and sizes.max() > 50000
    for t, (got, w) in enumerate(zip(_files(blob, offsets), want)):
        assert got == w, (t, divmod(t, cols), KINDS[t % len(KINDS)], tiles[t].shape)
    assert total == offsets[-1] == sum(len(w) for w in want)
    assert np.all(blob[total:] == 0x5C) and len(blob) == total + GUARD


# ---- measure and capacity --------------------------------------------------------------------

def test_capacity_one_short_writes_nothing(L):
    tiles = [jl.case_array(k) for k in ("cells", "zeros", "stripes")]
    _, _, measured, total = _encode(L, _level(tiles, 1, 3), 1, 3, T, T, 95, write=False)
    assert np.all(np.diff(measured) > 0)
    with hip.DeviceBuffer.from_array(_level(tiles, 1, 3)) as d_level, \
            hip.DeviceBuffer.from_array(np.full(4, -1, dtype=np.int64)) as d_off, \
            hip.DeviceBuffer.from_array(np.full(total + GUARD, 0x5C, dtype=np.uint8)) as d_out:
        got = C.c_int64(-1)
        rc = L.tmh_jpeg_encode_level_device(d_level, 1, 3, T, T, 95, d_out, total - 1, d_off,
                                            C.byref(got), None)
        assert rc == hip.TMH_EINVAL and len(L.tmh_last_error()) > 0
        assert got.value == total and np.array_equal(d_off.get(4, np.int64), measured)
        assert np.all(d_out.get(total + GUARD, np.uint8) == 0x5C), "a refused call wrote output"
        rc = L.tmh_jpeg_encode_level_device(d_level, 1, 3, T, T, 95, d_out, total, d_off,
                                            C.byref(got), None)
        assert rc == 0 and got.value == total
        blob = d_out.get(total + GUARD, np.uint8)
        assert np.all(blob[total:] == 0x5C) and blob[total - 2:total].tolist() == [0xFF, 0xD9]


# ---- bad arguments ------------------------------------------------------------------------------

def test_bad_arguments_launch_nothing(L):
    d_level = hip.DeviceBuffer.from_array(_level([jl.case_array("cells")] * 2, 1, 2))
    d_off = hip.DeviceBuffer.from_array(np.full(3, -7, dtype=np.int64))
    d_out = hip.DeviceBuffer.from_array(np.full(4096, 0x5C, dtype=np.uint8))
    total = C.c_int64(-7)

    def call(level=d_level, r=1, c=2, h=T, w=T, out=d_out, cap=4096, off=d_off,
             tot=C.byref(total)):
        return L.tmh_jpeg_encode_level_device(level, r, c, h, w, 95, out, cap, off, tot, None)

    host = np.zeros((T, T), dtype=np.uint8)
    hoff = np.full(2, -7, dtype=np.int64)
    bad = {
        "NULL level": lambda: call(level=None),
        "NULL offsets": lambda: call(off=None),
        "NULL total": lambda: call(tot=None),
        "rows 0": lambda: call(r=0),
        "cols negative": lambda: call(c=-1),
        "last height 0": lambda: call(h=0),
        "last height 257": lambda: call(h=257),
        "last width 0": lambda: call(w=0),
        "last width 257": lambda: call(w=257),
        "host form NULL level": lambda: L.tmh_jpeg_encode_level(
            None, 1, 1, T, T, 95, None, 0, hip.ptr(hoff), C.byref(total)),
        "host form last width 300": lambda: L.tmh_jpeg_encode_level(
            hip.ptr(host), 1, 1, T, 300, 95, None, 0, hip.ptr(hoff), C.byref(total)),
    }
    with d_level, d_off, d_out:
        for name, f in bad.items():
            assert f() == hip.TMH_EINVAL, name
            assert len(L.tmh_last_error()) > 0, name
        hip.check(L.tmh_synchronize(None))
        assert total.value == -7 and np.all(hoff == -7)
        assert np.all(d_off.get(3, np.int64) == -7), "a refused call wrote offsets"
        assert np.all(d_out.get(4096, np.uint8) == 0x5C), "a refused call wrote output"


# ---- quality clamp --------------------------------------------------------------------------------

def test_quality_is_clamped_like_libjpeg(L, literal):
    a = jl.case_array("cells", (96, 72))
    level = _level([a], 1, 1)
    got = {q: _encode(L, level, 1, 1, 96, 72, q)[1][:-GUARD].tobytes() for q in (0, -5, 1, 100, 101, 1000)}
    assert got[0] == got[-5] == got[1] == literal(a, 1)
    assert got[101] == got[1000] == got[100] == literal(a, 100)
    assert got[1] != got[100]


# ---- larger count ------------------------------------------------------------------------------------

def test_three_hundred_noise_tiles(L, literal):
    """A 12 x 25 level of seeded noise at quality 95: more tiles than CUs,
    offsets that pass 2^24.  The 300 tiles are drawn (seeded) from 16 distinct
    noise tiles, so the literal codes 16 tiles and not 300 (tens of ms each)."""
    rng = np.random.default_rng(300)
    distinct = [jl.case_array("noise", (T, T), seed=50 + i) for i in range(16)]
    pick = rng.integers(0, len(distinct), 300)
    _, blob, offsets, total = _encode(L, _level([distinct[i] for i in pick], 12, 25), 12, 25, T, T, 95)
    want = [literal(distinct[i]) for i in pick]
    assert len({len(literal(a)) for a in distinct}) > 1
    assert offsets.tolist() == np.concatenate([[0], np.cumsum([len(w) for w in want])]).tolist()
    assert total == offsets[-1] > 1 << 24
    assert hashlib.sha256(blob[:total].tobytes()).hexdigest() == \
        hashlib.sha256(b"".join(want)).hexdigest()
    assert np.all(blob[total:] == 0x5C)


# ---- Python layer ----------------------------------------------------------------------------------------

def test_pyramid_encode_level_and_iter(L, literal):
    from tmlibrary_amd.workflow.pyramid import EncodedLevel, build_pyramid
    g = lit.make_layer("one_well")
    sites = lit.random_sites(g)
    with build_pyramid(g, sites) as pyr:
        want = {}
        for z in range(pyr.depth):
            enc = pyr.encode_level(z)
            rows, cols = pyr.dimensions[z]
            assert isinstance(enc, EncodedLevel) and enc.dimensions == (rows, cols)
            assert enc.blob.dtype == np.uint8 and enc.blob.ndim == 1
            assert enc.offsets.dtype == np.int64 and enc.offsets.shape == (rows * cols + 1,)
            assert enc.offsets[0] == 0 and enc.offsets[-1] == len(enc.blob)
            for y in range(rows):
                for x in range(cols):
                    want[(z, y, x)] = literal(pyr.tile(z, y, x).array)
                    got = enc.tile(y, x)
                    assert isinstance(got, bytes) and got == want[(z, y, x)], (z, y, x)
            with pytest.raises(IndexError):
                enc.tile(rows, 0)
        assert pyr.tile(0, 0, 0).dimensions != (T, T)       # ragged levels are part of it
        rows_ = list(pyr.iter_jpeg_tiles())
        order = [(z, y, x) for z in range(pyr.depth - 1, -1, -1)
                 for y in range(pyr.dimensions[z][0]) for x in range(pyr.dimensions[z][1])]
        assert [r[:3] for r in rows_] == order and len(rows_) == g.n_tiles
        assert all(r[3] == want[r[:3]] for r in rows_)
        q50 = pyr.encode_level(0, quality=50).tile(0, 0)
        assert q50 == literal(pyr.tile(0, 0, 0).array, 50)
        with pytest.raises(IndexError):
            pyr.encode_level(pyr.depth)
    with pytest.raises(ValueError):
        pyr.encode_level(0)      # closed


def test_pyramid_tile_jpeg_encode(L, literal):
    from tmlibrary_amd.image import PyramidTile
    a = jl.case_array("cells", (37, 101))
    got = PyramidTile(a).jpeg_encode()
    assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and got.ndim == 1
    assert got.tobytes() == literal(a, 95)
    assert PyramidTile(a).jpeg_encode(quality=30).tobytes() == literal(a, 30)
    full = PyramidTile.create_as_background().jpeg_encode()
    assert len(full) == 1100 and full.tobytes() == literal(np.zeros((T, T), np.uint8))
