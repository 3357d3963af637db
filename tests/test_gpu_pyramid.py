"""GPU: the illuminati tile pyramid through the C-ABI -- the base-tile gather
(k_tiles_base), the level halving (k_pyramid_shrink2), ``build_pyramid`` /
``Pyramid`` and ``Image.shrink``.  Everything is bit-exact against the literal
numpy restatement of the reference's loops in tests/pyramid_literal.py."""
import ctypes as C
import itertools

import numpy as np
import pytest

import pyramid_literal as lit
from tmlibrary_amd import hip
from util import keep  # noqa: F401 (a fixture)

pytestmark = pytest.mark.gpu
T = 256


@pytest.fixture(scope="module")
def L():
    return hip.lib()


@pytest.fixture(scope="module")
def cases():
    """Per layer (built once, never modified): geometry, random sites, the
    literal base level and its missing tiles."""
    cache = {}

    def get(name):
        if name not in cache:
            g = lit.make_layer(name)
            sites = lit.random_sites(g)
            want, missing = lit.literal_base_level(g, sites)
            for a in (sites, want):
                a.flags.writeable = False
            cache[name] = (g, sites, want, missing)
        return cache[name]
    return get


def _stitch(level):
    from tmlibrary_amd.image import tiles_to_array
    return tiles_to_array(level, T, T)


# ---- base tiles -------------------------------------------------------------------

@pytest.mark.parametrize("name", lit.CPU_LAYERS + ("production_pitch",))
def test_base_tiles_match_literal_loop(L, cases, name):
    from tmlibrary_amd.workflow.pyramid import build_pyramid
    g, sites, want, missing = cases(name)
    with build_pyramid(g, sites) as pyr:
        z = pyr.depth - 1
        assert z == g.maxzoom_level_index and pyr.dimensions[z] == want.shape[:2]
        got = pyr.level(z)
        assert got.shape == (want.shape[0] * T, want.shape[1] * T)
        assert np.array_equal(got, _stitch(want))
        assert pyr.empty_base_tiles == missing
        for r, c in sorted(missing)[:4]:
            t = pyr.tile(z, r, c)
            assert t.dimensions == (T, T) and not t.array.any()   # spacer tiles are all zero
    if name == "two_wells":
        assert len(missing) > 0
    if name == "production_pitch":
        assert g.image_size[1] == 2560 and want.shape[:2] == (17, 30)


def test_tiles_base_host_form_any_table_order(L, cases):
    """tmh_tiles_base (host pointers) with the table shuffled: the entry
    point sorts by tile itself."""
    from tmlibrary_amd.workflow.pyramid import plan_base_tiles
    g, sites, want, _ = cases("two_wells")
    table = plan_base_tiles(g)
    table = np.ascontiguousarray(table[np.random.default_rng(3).permutation(len(table))])
    rows, cols = g.dimensions[-1]
    out = np.full((rows, cols, T, T), 0xAA, dtype=np.uint8)
    src = np.ascontiguousarray(sites)
    hip.check(L.tmh_tiles_base(hip.ptr(src), len(src), src.shape[1], src.shape[2], hip.ptr(table),
                               len(table), hip.ptr(out), rows, cols))
    assert np.array_equal(out, want)


# ---- shrink -------------------------------------------------------------------------

def _shrink_host_form(L, level, last_h, last_w, fill=0xAA):
    rows, cols = level.shape[:2]
    out = np.full(((rows + 1) // 2, (cols + 1) // 2, T, T), fill, dtype=np.uint8)
    oh, ow = C.c_int(-1), C.c_int(-1)
    src = np.ascontiguousarray(level)
    hip.check(L.tmh_pyramid_shrink2(hip.ptr(src), rows, cols, last_h, last_w, hip.ptr(out),
                                    C.byref(oh), C.byref(ow)))
    return out, oh.value, ow.value


def _shrink_device_form(L, level, last_h, last_w, fill=0xAA):
    rows, cols = level.shape[:2]
    oshape = ((rows + 1) // 2, (cols + 1) // 2, T, T)
    with hip.DeviceBuffer.from_array(level) as src, \
            hip.DeviceBuffer.from_array(np.full(oshape, fill, np.uint8)) as dst:
        oh, ow = C.c_int(-1), C.c_int(-1)
        hip.check(L.tmh_pyramid_shrink2_device(src, rows, cols, last_h, last_w, dst,
                                               C.byref(oh), C.byref(ow), None))
        hip.check(L.tmh_synchronize(None))
        return dst.get(oshape, np.uint8), oh.value, ow.value


def test_shrink_rounding_every_block(L):
    """A 2 x 2-tile level whose 2 x 2 pixel blocks enumerate {0, 1, 2, 254, 255}^4
    (the issue's {0, 1, 2, 255} plus the 254 its own half-way case 255, 255,
    255, 254 needs): (a + b + c + d + 2) >> 2, half-way cases rounding up."""
    vals = np.array(list(itertools.product((0, 1, 2, 254, 255), repeat=4)), dtype=np.uint8)
    idx = np.arange(256 * 256).reshape(256, 256) % len(vals)       # all 625 blocks, many times
    mosaic = np.zeros((512, 512), dtype=np.uint8)
    mosaic[0::2, 0::2] = vals[idx, 0]
    mosaic[0::2, 1::2] = vals[idx, 1]
    mosaic[1::2, 0::2] = vals[idx, 2]
    mosaic[1::2, 1::2] = vals[idx, 3]
    from tmlibrary_amd.image import array_to_tiles
    level, lh, lw = array_to_tiles(mosaic)
    assert level.shape[:2] == (2, 2) and (lh, lw) == (T, T)
    out, oh, ow = _shrink_host_form(L, level, lh, lw)
    assert (oh, ow) == (T, T) and out.shape == (1, 1, T, T)
    s = vals.astype(np.int64).sum(axis=1)
    want = ((s + 2) >> 2).astype(np.uint8)[idx]
    assert np.array_equal(out[0, 0], want)
    k = [tuple(v) for v in vals.tolist()]
    assert out[0, 0].ravel()[k.index((1, 0, 0, 1))] == 1          # 2 / 4 -> 1
    assert out[0, 0].ravel()[k.index((255, 255, 255, 254))] == 255   # 1019 / 4 -> 255
    assert out[0, 0].ravel()[k.index((1, 0, 0, 0))] == 0


@pytest.mark.parametrize("last", [(128, 64), (2, 2), (256, 256)])
def test_shrink_ragged_levels(L, last):
    """3 x 5 source tiles with a ragged last row / column against join-then-
    shrink (api.py:513-568), through the device entry point."""
    lh, lw = last
    rng = np.random.default_rng(lh * 7 + lw)
    full = rng.integers(0, 256, (2 * T + lh, 4 * T + lw), dtype=np.uint8)
    from tmlibrary_amd.image import array_to_tiles
    level, a, b = array_to_tiles(full)
    assert level.shape[:2] == (3, 5) and (a, b) == last
    want_tiles, orows, ocols = lit.literal_lower_level(lit.level_to_dict(level, lh, lw), 3, 5)
    want = lit.dict_to_level(want_tiles, orows, ocols)
    got, oh, ow = _shrink_device_form(L, level, lh, lw)
    assert (oh, ow) == want_tiles[(orows - 1, ocols - 1)].shape == (lh // 2, lw // 2)
    assert np.array_equal(got, want)      # whole tiles: zeros outside the ragged extent
    got2, oh2, ow2 = _shrink_host_form(L, level, lh, lw)
    assert (oh2, ow2) == (oh, ow) and np.array_equal(got2, want)


def test_shrink_leaves_odd_mosaics_to_the_host(L):
    """A 2 x 4-tile level with last column width 1: output column 1's mosaics
    are 257 wide; the device entry leaves those tiles untouched."""
    rng = np.random.default_rng(11)
    full = rng.integers(0, 256, (2 * T, 3 * T + 1), dtype=np.uint8)
    from tmlibrary_amd.image import array_to_tiles, Image
    level, lh, lw = array_to_tiles(full)
    assert level.shape[:2] == (2, 4) and (lh, lw) == (T, 1)
    got, oh, ow = _shrink_device_form(L, level, lh, lw, fill=0x5C)
    assert (oh, ow) == (T, 128) and got.shape == (1, 2, T, T)
    assert np.array_equal(got[0, 0], lit.shrink_even(full[:, :512]))
    assert np.all(got[0, 1] == 0x5C), "the odd mosaic's tile must not be written"
    # the Python interface completes it: Image.shrink of the odd mosaic on the host ...
    odd = Image(np.ascontiguousarray(full[:, 512:])).shrink(2, inplace=False).array
    assert odd.shape == (T, 128) and np.array_equal(odd, lit.exact_half(full[:, 512:]))
    # ... and of an even image on the device
    even = Image(full[:, :600].copy())
    assert even.shrink(2) is even and np.array_equal(even.array, lit.shrink_even(full[:, :600]))


def test_pyramid_with_an_odd_level_is_complete(L):
    """A layer 2 x 257 tiles wide: nine levels up a level is 257 pixels wide
    (two tiles, the last one pixel wide) and its mosaic odd -- build_pyramid
    fills that tile on the host."""
    from tmlibrary_amd.workflow.pyramid import LayerGeometry, build_pyramid
    sites = [(0, y, x, (y * T, x * T)) for y in range(2) for x in range(257)]
    g = LayerGeometry((T, T), sites, {0: (2, 257)})
    assert g.depth == 10 and g.dimensions[1] == (1, 2) and g.dimensions[0] == (1, 1)
    px = lit.random_sites(g, seed=99)
    tiles, missing = lit.literal_base_level(g, px)
    assert not missing
    tiles, rows, cols = lit.level_to_dict(tiles), 2, 257
    with build_pyramid(g, px) as pyr:
        for z in range(pyr.depth - 2, -1, -1):
            tiles, rows, cols = lit.literal_lower_level(tiles, rows, cols)
            assert (rows, cols) == pyr.dimensions[z]
            if z <= 1:
                for (r, c), want in tiles.items():
                    assert np.array_equal(pyr.tile(z, r, c).array, want), (z, r, c)
        assert pyr.tile(1, 0, 1).dimensions == (2, 1)
        assert pyr.tile(0, 0, 0).dimensions == (1, 128)     # floor(257 / 2) wide
        assert pyr.level(0).shape == (1, 128)


# ---- whole pyramid ----------------------------------------------------------------------

def test_whole_pyramid_two_wells(L, cases):
    from tmlibrary_amd.image import PyramidTile
    from tmlibrary_amd.workflow.pyramid import build_pyramid
    g, sites, want, _ = cases("two_wells")
    sizes = g._get_image_sizes(g.height, g.width)
    with build_pyramid(g, sites) as pyr:
        assert pyr.depth == len(sizes) == g.depth
        assert pyr.dimensions == [(-(-h // T), -(-w // T)) for h, w in sizes] == g.dimensions
        assert pyr.dimensions[0] == (1, 1)
        rows, cols = pyr.dimensions[-1]
        tiles = lit.level_to_dict(want)
        for z in range(pyr.depth - 1, -1, -1):
            if z < pyr.depth - 1:
                tiles, rows, cols = lit.literal_lower_level(tiles, rows, cols)
            assert (rows, cols) == pyr.dimensions[z]
            for (r, c), w in tiles.items():
                t = pyr.tile(z, r, c)
                assert isinstance(t, PyramidTile) and t.dimensions == w.shape, (z, r, c)
                assert np.array_equal(t.array, w), (z, r, c)
                assert (t.metadata.z, t.metadata.y, t.metadata.x) == (z, r, c)
            stitched = np.vstack([np.hstack([tiles[(r, c)] for c in range(cols)])
                                  for r in range(rows)])
            assert np.array_equal(pyr.level(z), stitched)
        # ragged sizes: 7 x 12 base tiles halve to 4 x 6 (last row 128 high), 2 x 3 (192),
        # 1 x 2 (224 x 128) and the top tile of 112 x 192
        assert pyr.dimensions == [(1, 1), (1, 2), (2, 3), (4, 6), (7, 12)]
        assert pyr.tile(3, 3, 5).dimensions == (128, 256)
        assert pyr.tile(2, 1, 2).dimensions == (192, 256)
        assert pyr.tile(1, 0, 1).dimensions == (224, 128)
        assert pyr.tile(0, 0, 0).dimensions == (112, 192)
        with pytest.raises(IndexError):
            pyr.tile(1, 1, 0)
    with pytest.raises(ValueError):
        pyr.tile(0, 0, 0)      # closed


# ---- device-resident path ------------------------------------------------------------------

def test_chain_output_feeds_the_pyramid_on_the_device(L, keep):
    """tmh_correct_chain_u8_device's device output goes straight into
    build_pyramid; same pyramid as from the host copy of that output."""
    from tmlibrary_amd.image import Corrector, align_window
    from tmlibrary_amd.synth import synth_sites_host
    from tmlibrary_amd.workflow.pyramid import build_pyramid
    g = lit.make_layer("one_well")
    n, (H, W) = len(g.sites), g.image_size
    raw = np.ascontiguousarray(synth_sites_host(n, H, W, seed=5))
    yy, xx = np.mgrid[0:H, 0:W]
    mean = 2.2 + 0.1 * np.cos(yy / 97.0) * np.sin(xx / 131.0)
    std = 0.25 + 0.02 * np.sin(yy / 53.0 + xx / 71.0)
    win = np.ascontiguousarray(np.array(
        [align_window((H, W), 3 - i, i - 2, 4, 4, 4, 4, crop=False)[0] for i in range(n)],
        dtype=hip.WINDOW_DTYPE))
    corr = Corrector(mean, std)
    d_in = keep(hip.DeviceBuffer.from_array(raw))
    d_out = keep(hip.DeviceBuffer.from_array(np.full(n * H * W, 0xAA, np.uint8)))
    try:
        hip.check(L.tmh_correct_chain_u8_device(corr._h, d_in, d_out, n, hip.ptr(win), 110, 900,
                                                None))
        with build_pyramid(g, d_out.ptr) as from_device:
            host_copy = d_out.get((n, H, W), np.uint8)
            assert len(np.unique(host_copy)) > 100      # a real image, not a constant
            with build_pyramid(g, host_copy) as from_host:
                for z in range(from_host.depth):
                    assert np.array_equal(from_device.level(z), from_host.level(z)), z
            want, _ = lit.literal_base_level(g, host_copy)
            assert np.array_equal(from_device.level(from_device.depth - 1), _stitch(want))
    finally:
        corr.close()


# ---- argument errors --------------------------------------------------------------------------

def test_argument_errors_launch_nothing(L):
    n, H, W, rows, cols = 2, 300, 420, 2, 2
    sites = hip.DeviceBuffer.from_array(np.full(n * H * W, 7, np.uint8))
    tiles = hip.DeviceBuffer.from_array(np.full(rows * cols * T * T, 0xAA, np.uint8))
    small = hip.DeviceBuffer.from_array(np.full(T * T, 0xAA, np.uint8))
    ok = (1, 1, 10, 20, 30, 40, 50, 60)

    def table(*recs):
        return np.array(list(recs), dtype=hip.TILE_RECT_DTYPE)

    def base(sites_p=sites, n_sites=n, h=H, w=W, recs=table(ok), n_rects=None, tiles_p=tiles,
             tr=rows, tc=cols):
        rp = None if recs is None else hip.ptr(recs)
        nr = (0 if recs is None else len(recs)) if n_rects is None else n_rects
        return L.tmh_tiles_base_device(sites_p, n_sites, h, w, rp, nr, tiles_p, tr, tc, None)

    def change(**kw):
        r = dict(zip(hip.TILE_RECT_DTYPE.names, ok))
        r.update(kw)
        return table(tuple(r[k] for k in hip.TILE_RECT_DTYPE.names))

    lh, lw = C.c_int(), C.c_int()

    def shrink(src=tiles, r=rows, c=cols, h=T, w=T, dst=small, ph=C.byref(lh), pw=C.byref(lw)):
        return L.tmh_pyramid_shrink2_device(src, r, c, h, w, dst, ph, pw, None)

    bad = {
        "NULL sites": lambda: base(sites_p=None),
        "NULL tiles": lambda: base(tiles_p=None),
        "NULL table": lambda: base(recs=None, n_rects=1),
        "leaves site (rows)": lambda: base(recs=change(src_y=H - 49)),
        "leaves site (columns)": lambda: base(recs=change(src_x=W - 59)),
        "negative source": lambda: base(recs=change(src_x=-1)),
        "leaves tile (rows)": lambda: base(recs=change(dst_y=T - 49)),
        "leaves tile (columns)": lambda: base(recs=change(dst_x=T - 59)),
        "negative destination": lambda: base(recs=change(dst_y=-1)),
        "tile index high": lambda: base(recs=change(tile=rows * cols)),
        "tile index negative": lambda: base(recs=change(tile=-1)),
        "site index high": lambda: base(recs=change(site=n)),
        "site index negative": lambda: base(recs=change(site=-1)),
        "rect height 0": lambda: base(recs=change(height=0)),
        "rect width negative": lambda: base(recs=change(width=-3)),
        "no sites": lambda: base(n_sites=0),
        "height 0": lambda: base(h=0),
        "width negative": lambda: base(w=-1),
        "tile rows 0": lambda: base(tr=0),
        "tile cols 0": lambda: base(tc=0),
        "second record bad": lambda: base(recs=table(ok, (0, 0, 0, 0, 0, 0, 257, 1))),
        "shrink NULL source": lambda: shrink(src=None),
        "shrink NULL output": lambda: shrink(dst=None),
        "shrink NULL height": lambda: shrink(ph=None),
        "shrink NULL width": lambda: shrink(pw=None),
        "shrink rows 0": lambda: shrink(r=0),
        "shrink cols negative": lambda: shrink(c=-2),
        "shrink last height 0": lambda: shrink(h=0),
        "shrink last width 257": lambda: shrink(w=257),
        "shrink in place": lambda: shrink(dst=tiles),
    }
    with sites, tiles, small:
        for name, call in bad.items():
            assert call() == hip.TMH_EINVAL, name
            assert len(L.tmh_last_error()) > 0, name
        hip.check(L.tmh_synchronize(None))
        assert np.all(tiles.get(rows * cols * T * T, np.uint8) == 0xAA), "a refused call wrote tiles"
        assert np.all(small.get(T * T, np.uint8) == 0xAA), "a refused call wrote a level"
        # the same calls with good arguments do run
        assert base() == hip.TMH_OK
        got = tiles.get((rows * cols, T, T), np.uint8)
        want = np.zeros_like(got)
        want[1, 30:80, 40:100] = 7
        assert np.array_equal(got, want)
        assert shrink() == hip.TMH_OK and (lh.value, lw.value) == (T, T)
        hip.check(L.tmh_synchronize(None))
        assert np.array_equal(small.get((T, T), np.uint8),
                              lit.shrink_even(np.vstack([np.hstack([got[0], got[1]]),
                                                         np.hstack([got[2], got[3]])])))
