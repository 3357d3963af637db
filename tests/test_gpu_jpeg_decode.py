"""GPU: JPEG decoding of pyramid tiles -- the round trip of a level
(k_jpeg_roundtrip), the decoder of stored files (k_jpeg_decode_tiles) and the
stored pyramid ``build_pyramid(jpeg_quality=...)`` on top of them.  Everything
is exact: against what libjpeg-turbo decoded (tests/golden/jpeg_decoded.npz;
no test here imports Pillow) and against tests/jpeg_decode_literal.py, which
the CPU suite pins to it.  The files that must be refused are the ones
tests/test_jpeg_decode_cpu.py has already run through the same decoder code
on the CPU, under sanitizers.
"""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest

import jpeg_decode_literal as jd
import jpeg_literal as jl
import pyramid_literal as lit
from tmlibrary_amd import hip
from util import REPO

pytestmark = pytest.mark.gpu
T = 256
GOLDEN = os.path.join(REPO, "tests", "golden", "jpeg_decoded.npz")


@pytest.fixture(scope="module")
def L():
    return hip.lib()


@pytest.fixture(scope="module")
def goldens():
    return jd.load_goldens(GOLDEN)


def _level(tiles, surround=0):
    level = np.full((len(tiles), T, T), surround, dtype=np.uint8)
    for t, a in enumerate(tiles):
        level[t, :a.shape[0], :a.shape[1]] = a
    return level


def _roundtrip_device(L, level, rows, cols, last_h, last_w, quality):
    with hip.DeviceBuffer.from_array(level) as d_in, \
            hip.DeviceBuffer.from_array(np.full(level.shape, 0x5C, dtype=np.uint8)) as d_out:
        hip.check(L.tmh_jpeg_roundtrip_level_device(d_in, rows, cols, last_h, last_w, quality,
                                                    d_out, None))
        hip.check(L.tmh_synchronize(None))
        assert np.array_equal(d_in.get(level.shape, np.uint8), level), "the input was written"
        return d_out.get(level.shape, np.uint8)


def _mixed_level():
    """3 x 2 tiles, last row 37 high, last column 101 wide, mixed kinds with a
    one-value tile; 0xAA around the ragged tiles."""
    rows, cols, lh, lw = 3, 2, 37, 101
    kinds = ("cells", "noise", "full", "stripes", "specks", "smooth")
    tiles = [jl.case_array(kinds[t], (lh if t // cols == rows - 1 else T,
                                      lw if t % cols == cols - 1 else T), seed=40 + t)
             for t in range(rows * cols)]
    return tiles, rows, cols, lh, lw


@pytest.fixture(scope="module")
def mixed():
    tiles, rows, cols, lh, lw = _mixed_level()
    return tiles, rows, cols, lh, lw, [jd.roundtrip(a, 95) for a in tiles]


# ---- the round trip of a level -----------------------------------------------------------

def test_roundtrip_every_golden_as_a_one_tile_level(L, goldens):
    for name, a, q, _, want in goldens:
        h, w = a.shape
        level = _level([a], surround=0xAA)
        got = _roundtrip_device(L, level, 1, 1, h, w, q)[0]
        assert np.array_equal(got[:h, :w], want), name
        assert not got[h:].any() and not got[:, w:].any(), name
        if name in ("cells", "ragged_9x17"):      # the host form
            out = np.full_like(level, 0x5C)
            hip.check(L.tmh_jpeg_roundtrip_level(hip.ptr(level), 1, 1, h, w, q, hip.ptr(out)))
            assert np.array_equal(out[0], got), name


def test_roundtrip_mixed_ragged_level(L, mixed):
    tiles, rows, cols, lh, lw, want = mixed
    got = _roundtrip_device(L, _level(tiles, surround=0xAA), rows, cols, lh, lw, 95)
    for t, (a, w) in enumerate(zip(tiles, want)):
        h, wd = a.shape
        assert np.array_equal(got[t, :h, :wd], w), (t, a.shape)
        assert not got[t, h:].any() and not got[t, :, wd:].any(), (t, "zeros around the tile")
    assert len(np.unique(tiles[2])) == 1                            # the one-value tile


def test_roundtrip_one_by_one_level(L):
    a = np.array([[201]], dtype=np.uint8)
    got = _roundtrip_device(L, _level([a], surround=0xAA), 1, 1, 1, 1, 95)
    assert got[0, 0, 0] == jd.roundtrip(a, 95)[0, 0] and got.sum() == got[0, 0, 0]


def test_roundtrip_bad_arguments_launch_nothing(L):
    d_in = hip.DeviceBuffer.from_array(_level([jl.case_array("cells")] * 2))
    d_out = hip.DeviceBuffer.from_array(np.full((2, T, T), 0x5C, dtype=np.uint8))

    def call(level=d_in, r=1, c=2, h=T, w=T, out=d_out):
        return L.tmh_jpeg_roundtrip_level_device(level, r, c, h, w, 95, out, None)

    host = np.zeros((T, T), dtype=np.uint8)
    hout = np.full((T, T), 0x5C, dtype=np.uint8)
    bad = {
        "NULL level": lambda: call(level=None),
        "NULL output": lambda: call(out=None),
        "in place": lambda: call(out=d_in),
        "rows 0": lambda: call(r=0),
        "cols negative": lambda: call(c=-1),
        "last height 0": lambda: call(h=0),
        "last height 257": lambda: call(h=257),
        "last width 0": lambda: call(w=0),
        "last width 257": lambda: call(w=257),
        "host form NULL level": lambda: L.tmh_jpeg_roundtrip_level(None, 1, 1, T, T, 95, hip.ptr(hout)),
        "host form last width 300": lambda: L.tmh_jpeg_roundtrip_level(
            hip.ptr(host), 1, 1, T, 300, 95, hip.ptr(hout)),
    }
    with d_in, d_out:
        for name, f in bad.items():
            assert f() == hip.TMH_EINVAL, name
            assert len(L.tmh_last_error()) > 0, name
        hip.check(L.tmh_synchronize(None))
        assert np.all(d_out.get((2, T, T), np.uint8) == 0x5C) and np.all(hout == 0x5C), \
            "a refused call wrote output"


# ---- the decoder of files -----------------------------------------------------------------

def _decode_device(L, files):
    """One call of the device entry -> (tiles [n][256][256], dims, status)."""
    n = len(files)
    offsets = np.concatenate([[0], np.cumsum([len(f) for f in files])]).astype(np.int64)
    blob = np.frombuffer(b"".join(files), np.uint8)
    with contextlib.ExitStack() as stack:
        def upload(a):
            d = stack.enter_context(hip.DeviceBuffer(max(a.nbytes, 16)))
            d.put(a)
            return d
        d_blob, d_off = upload(blob), upload(offsets)
        d_tiles = upload(np.full((n + 1, T, T), 0x5C, dtype=np.uint8))      # one tile of guard
        d_dims, d_status = upload(np.full((n, 2), -7, np.int32)), upload(np.full(n, -7, np.int32))
        hip.check(L.tmh_jpeg_decode_tiles_device(d_blob, d_off, n, d_tiles, d_dims,
                                                 d_status, None))
        tiles = d_tiles.get((n + 1, T, T), np.uint8)
        assert np.all(tiles[n] == 0x5C), "a write past the last tile"
        return tiles[:n], d_dims.get((n, 2), np.int32), d_status.get(n, np.int32)


def test_decode_every_golden_in_one_call(L, goldens):
    files = [g[3] for g in goldens]
    tiles, dims, status = _decode_device(L, files)
    assert not status.any()
    for t, (name, _, _, _, want) in enumerate(goldens):
        h, w = want.shape
        assert dims[t].tolist() == [h, w], name
        assert np.array_equal(tiles[t, :h, :w], want), name
        assert not tiles[t, h:].any() and not tiles[t, :, w:].any(), name
    # the host form gives the same
    n = len(files)
    offsets = np.concatenate([[0], np.cumsum([len(f) for f in files])]).astype(np.int64)
    blob = np.frombuffer(b"".join(files), np.uint8)
    h_tiles = np.full((n, T, T), 0x5C, np.uint8)
    h_dims, h_status = np.full((n, 2), -7, np.int32), np.full(n, -7, np.int32)
    hip.check(L.tmh_jpeg_decode_tiles(hip.ptr(blob), hip.ptr(offsets), n, hip.ptr(h_tiles),
                                      hip.ptr(h_dims), hip.ptr(h_status)))
    assert np.array_equal(h_tiles, tiles) and np.array_equal(h_dims, dims) and not h_status.any()


def test_status_cases_among_good_files(L, goldens):
    """Every refused file gives the status the rules name, a tile of zeros and
    dims (0, 0); the good files between them still decode."""
    z = np.load(GOLDEN)
    base = [g for g in goldens if g[0] == "extra7"][0]
    bad = jd.status_cases(base[3], {k[4:]: z[k] for k in z.files if k.startswith("bad_")})
    good = jd.good_variants(base[3])
    files, want = [], []
    for i, (_, f, s) in enumerate(bad):
        files += [f, good[i % len(good)][1]]
        want += [s, 0]
    tiles, dims, status = _decode_device(L, files)
    assert status.tolist() == want
    h, w = base[4].shape
    for t, s in enumerate(want):
        if s:
            assert not tiles[t].any() and dims[t].tolist() == [0, 0], bad[t // 2][0]
        else:
            assert dims[t].tolist() == [h, w] and np.array_equal(tiles[t, :h, :w], base[4]), t
            assert not tiles[t, h:].any() and not tiles[t, :, w:].any(), t


def test_decode_empty_list_and_bad_arguments(L):
    from tmlibrary_amd.workflow.pyramid import decode_jpeg_tiles
    assert decode_jpeg_tiles([]) == []
    off = np.zeros(1, dtype=np.int64)
    assert L.tmh_jpeg_decode_tiles(None, hip.ptr(off), 0, None, None, None) == 0
    with hip.DeviceBuffer(max(off.nbytes, 16)) as d_off:
        d_off.put(off)
        assert L.tmh_jpeg_decode_tiles_device(None, d_off, 0, None, None, None, None) == 0
        assert L.tmh_jpeg_decode_tiles_device(None, d_off, 1, None, None, None, None) == hip.TMH_EINVAL
        assert L.tmh_jpeg_decode_tiles_device(None, None, 0, None, None, None, None) == hip.TMH_EINVAL
        assert L.tmh_jpeg_decode_tiles_device(None, d_off, -1, None, None, None, None) == hip.TMH_EINVAL
    blob, tile = np.zeros(8, np.uint8), np.full((T, T), 0x5C, np.uint8)
    dims, status = np.full(2, -7, np.int32), np.full(1, -7, np.int32)
    down = np.array([4, 2], dtype=np.int64)
    assert L.tmh_jpeg_decode_tiles(hip.ptr(blob), hip.ptr(down), 1, hip.ptr(tile), hip.ptr(dims),
                                   hip.ptr(status)) == hip.TMH_EINVAL
    assert len(L.tmh_last_error()) > 0
    assert np.all(tile == 0x5C) and np.all(dims == -7) and status[0] == -7


def test_decode_jpeg_tiles_raises_with_index_and_status(L, goldens):
    from tmlibrary_amd.workflow.pyramid import decode_jpeg_tiles
    by = {g[0]: g for g in goldens}
    files = [by["ragged_9x17"][3], np.frombuffer(by["extra3"][3], np.uint8), bytearray(by["zeros"][3])]
    got = decode_jpeg_tiles(files)
    for g, name in zip(got, ("ragged_9x17", "extra3", "zeros")):
        assert g.dtype == np.uint8 and np.array_equal(g, by[name][4]), name
    with pytest.raises(ValueError, match=r"file 1 is corrupt \(status 2\)"):
        decode_jpeg_tiles([files[0], files[0][:400], files[2]])
    with pytest.raises(ValueError, match=r"file 2 is unsupported \(status 1\)"):
        decode_jpeg_tiles([files[0], files[2], np.load(GOLDEN)["bad_progressive"]])


def test_encoded_level_decode_equals_the_roundtrip(L, mixed):
    """The decoder over the encoder's blob: an independent path to the same
    pixels as the round trip pass."""
    from tmlibrary_amd.image import tiles_to_array
    from tmlibrary_amd.workflow.pyramid import EncodedLevel
    tiles, rows, cols, lh, lw, want = mixed
    level = _level(tiles, surround=0xAA)
    n = rows * cols
    offsets, total = np.zeros(n + 1, np.int64), C.c_int64(0)
    hip.check(L.tmh_jpeg_encode_level(hip.ptr(level), rows, cols, lh, lw, 95, None, 0,
                                      hip.ptr(offsets), C.byref(total)))
    blob = np.empty(total.value, np.uint8)
    hip.check(L.tmh_jpeg_encode_level(hip.ptr(level), rows, cols, lh, lw, 95, hip.ptr(blob),
                                      blob.nbytes, hip.ptr(offsets), C.byref(total)))
    got = EncodedLevel(blob, offsets, (rows, cols)).decode()
    rt = np.full_like(level, 0x5C)
    hip.check(L.tmh_jpeg_roundtrip_level(hip.ptr(level), rows, cols, lh, lw, 95, hip.ptr(rt)))
    assert got.shape == ((rows - 1) * T + lh, (cols - 1) * T + lw)
    assert np.array_equal(got, tiles_to_array(rt.reshape(rows, cols, T, T), lh, lw))
    assert np.array_equal(got[:T, T:], want[1])


def test_pyramid_tile_create_from_binary_and_buffer(L):
    from tmlibrary_amd.image import PyramidTile
    from tmlibrary_amd.metadata import PyramidTileMetadata
    a = jl.case_array("cells", (37, 101))
    data = PyramidTile(a).jpeg_encode().tobytes()
    md = PyramidTileMetadata(1, 2, 3, None)
    tile = PyramidTile.create_from_binary(data, md)
    assert isinstance(tile, PyramidTile) and tile.metadata is md
    assert tile.array.dtype == np.uint8 and np.array_equal(tile.array, jd.roundtrip(a, 95))
    for buf in (data, bytearray(data), memoryview(data), np.frombuffer(data, np.uint8)):
        assert np.array_equal(PyramidTile.create_from_buffer(buf).array, tile.array)
    with pytest.raises(ValueError):
        PyramidTile.create_from_binary(data[:500])


# ---- the stored pyramid -------------------------------------------------------------------

@pytest.mark.parametrize("layer", ["one_well", "two_wells"])
def test_stored_pyramid(L, layer):
    """Every level against the stored-pyramid literal, and the files against
    jpeg_literal.encode of those levels (two_wells, which has spacer tiles and
    84 base tiles: the levels above the two largest -- the literal coder takes
    0.2 s a tile; the base level's pixels are checked like every level's)."""
    from tmlibrary_amd.workflow.pyramid import build_pyramid
    g = lit.make_layer(layer)
    sites = lit.random_sites(g)
    want = jd.stored_pyramid_literal(g, sites, 95)
    with build_pyramid(g, sites, jpeg_quality=95) as pyr:
        assert pyr.jpeg_quality == 95
        assert bool(pyr.empty_base_tiles) == (layer == "two_wells")
        for z in range(pyr.depth):
            tiles, rows, cols = want[z]
            assert pyr.dimensions[z] == (rows, cols)
            for (y, x), a in tiles.items():
                assert np.array_equal(pyr.tile(z, y, x).array, a), (z, y, x)
        for z in sorted({0, pyr.depth - 2}):
            tiles, rows, cols = want[z]
            dec = pyr.decoded_level(z)
            assert dec.shape == pyr.level(z).shape
            for (y, x), a in tiles.items():
                assert np.array_equal(dec[y * T:y * T + a.shape[0], x * T:x * T + a.shape[1]],
                                      jd.roundtrip(a, 95)), (z, y, x)
            assert np.array_equal(pyr.encode_level(z).decode(), dec)
        rows_ = list(pyr.iter_jpeg_tiles())
        assert [r[:3] for r in rows_] == [(z, y, x) for z in range(pyr.depth - 1, -1, -1)
                                          for y in range(pyr.dimensions[z][0])
                                          for x in range(pyr.dimensions[z][1])]
        coded = range(pyr.depth) if layer == "one_well" else range(pyr.depth - 2)
        for z, y, x, data in rows_:
            if z in coded:
                assert data == jl.encode(want[z][0][(y, x)], 95), (z, y, x)
        assert pyr.encode_level(0, quality=95).tile(0, 0) == rows_[-1][3]
        with pytest.raises(ValueError):
            pyr.encode_level(0, quality=90)
        with pytest.raises(ValueError):
            list(pyr.iter_jpeg_tiles(quality=50))


def test_stored_pyramid_odd_mosaic_reads_the_round_trip(L):
    """A layer 2 x 257 tiles wide (the smallest that reaches an odd-sided
    mosaic: base tiles are whole, so a level's width is 256 n / 2^k): level 1
    is 257 pixels wide and level 0's mosaic odd, finished on the host -- from
    the round trip of level 1, like the device pass.  The literal starts at
    level 2's pixels (514 base tiles through it would take several seconds)."""
    from tmlibrary_amd.workflow.pyramid import LayerGeometry, build_pyramid
    sites = [(0, y, x, (y * T, x * T)) for y in range(2) for x in range(257)]
    g = LayerGeometry((T, T), sites, {0: (2, 257)})
    px = lit.random_sites(g, seed=99)
    with build_pyramid(g, px, jpeg_quality=95) as pyr, build_pyramid(g, px) as direct:
        assert pyr.dimensions[2] == (1, 3) and pyr.tile(1, 0, 1).dimensions == (2, 1)
        tiles = {(0, x): pyr.tile(2, 0, x).array for x in range(3)}
        rows, cols = 1, 3
        for z in (1, 0):
            tiles = {k: jd.roundtrip(v, 95) for k, v in tiles.items()}
            tiles, rows, cols = lit.literal_lower_level(tiles, rows, cols)
            for (r, c), want in tiles.items():
                assert np.array_equal(pyr.tile(z, r, c).array, want), (z, r, c)
        assert pyr.level(0).shape == (1, 128)
        assert not np.array_equal(pyr.level(0), direct.level(0))


def test_no_jpeg_quality_builds_as_before(L):
    from tmlibrary_amd.workflow.pyramid import build_pyramid
    g = lit.make_layer("one_well")
    sites = lit.random_sites(g)
    direct = jd.stored_pyramid_literal(g, sites, None)
    with build_pyramid(g, sites) as a, build_pyramid(g, sites, jpeg_quality=None) as b:
        assert a.jpeg_quality is None and b.jpeg_quality is None
        differs = False
        for z in range(a.depth):
            la = a.level(z)
            assert np.array_equal(la, b.level(z))
            for (y, x), t in direct[z][0].items():
                assert np.array_equal(la[y * T:y * T + t.shape[0], x * T:x * T + t.shape[1]], t)
            differs = differs or not np.array_equal(a.decoded_level(z), la)
        assert differs
        assert a.encode_level(0).tile(0, 0) == a.encode_level(0, quality=95).tile(0, 0) == \
            jl.encode(direct[0][0][(0, 0)], 95)
        assert a.encode_level(0, quality=50).tile(0, 0) == jl.encode(direct[0][0][(0, 0)], 50)
