"""CPU: the host-only pieces of the illuminati tile pyramid -- the layer
geometry restated from tmlib/models/channel.py, the Image methods the tiling
uses, PyramidTile, the planner's rectangle table and the odd-side area mean.
No kernel is called (``hip.lib()`` refuses without a device).

References: fixtures generated from the reference itself
(tests/golden/make_pyramid_goldens.py) and, for the planner, the literal
restatement of the reference's loop in tests/pyramid_literal.py."""
import json
import os
from fractions import Fraction

import numpy as np
import pytest

from util import GOLDEN, load_golden
import pyramid_literal as lit
from tmlibrary_amd.image import Image, PyramidTile
from tmlibrary_amd.metadata import ImageMetadata, PyramidTileMetadata
from tmlibrary_amd.workflow import pyramid as P


@pytest.fixture(scope="module")
def geo():
    with open(os.path.join(GOLDEN, "pyramid_geometry.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def img():
    return load_golden("pyramid_image")


@pytest.fixture(scope="module")
def layer(geo):
    g = lit.make_layer("one_well")
    g._dimensions = [tuple(d) for d in geo["level_dimensions"]]  # the generator's stub levels
    return g


# ---- geometry vs the reference ------------------------------------------------

def test_tile_size_and_levels(layer):
    assert layer.tile_size == 256
    g = lit.make_layer("one_well")
    assert g.maxzoom_level_index == g.depth - 1 == len(g.dimensions) - 1


def test_calc_tile_indices_and_offsets(layer, geo):
    assert len(geo["indices_and_offsets"]) == 5 * 3 * 2
    for case in geo["indices_and_offsets"]:
        got = layer._calc_tile_indices_and_offsets(*case["args"])
        assert sorted(got) == ["indices", "offsets"]
        assert list(got["indices"]) == case["indices"], case["args"]
        assert list(got["offsets"]) == case["offsets"], case["args"]


def test_calc_tile_indices(layer, geo):
    for case in geo["indices"]:
        assert list(layer._calc_tile_indices(*case["args"])) == case["indices"], case["args"]


def test_get_image_sizes_and_dimensions(geo):
    for case in geo["image_sizes"]:
        h, w = case["args"]
        g = P.LayerGeometry((256, 256), [(0, 0, 0, (0, 0))], {0: (1, 1)}, layer_size=(h, w))
        sizes = g._get_image_sizes(h, w)
        assert [list(s) for s in sizes] == case["sizes"]
        assert all(isinstance(s, tuple) for s in sizes)
        assert g.depth == len(sizes)
        assert g.dimensions == [(-(-a // 256), -(-b // 256)) for a, b in sizes]


def test_calc_coordinates_of_next_higher_level(layer, geo):
    for case in geo["next_higher"]:
        got = layer.calc_coordinates_of_next_higher_level(*case["args"])
        assert [list(c) for c in got] == case["coordinates"], case["args"]


def test_extract_tile_from_image(layer, img):
    site = img["site"]
    for k, (yo, xo) in enumerate(img["tile_offsets"]):
        t = layer.extract_tile_from_image(Image(site), int(yo), int(xo))
        assert isinstance(t, PyramidTile)
        assert np.array_equal(t.array, img["tile_%d" % k]), (yo, xo)
        assert np.array_equal(lit.literal_extract_tile(site, int(yo), int(xo)), img["tile_%d" % k])


def test_neighbour_maps_one_well():
    """map_image_to_base_tiles / map_base_tile_to_images on the 2 x 3 well (the
    reference's two methods query a database session; restated by reading)."""
    g = lit.make_layer("one_well")
    assert g.dimensions[-1] == (3, 5) and (g.height, g.width) == (600, 1260)
    first = g.map_image_to_base_tiles(0)
    # site (0, 0): tile (0, 0) only -- row 1 and column 1 overhang and have neighbours
    assert first == [{'y': 0, 'x': 0, 'y_offset': 0, 'x_offset': 0}]
    last = g.map_image_to_base_tiles(5)      # site (1, 2) at (300, 840): well's lower right
    assert [(t['y'], t['x']) for t in last] == [(1, 3), (1, 4), (2, 3), (2, 4)]
    assert last[0]['y_offset'] == 256 - 300 and last[0]['x_offset'] == 3 * 256 - 840
    extra = g.map_base_tile_to_images(5)
    assert sorted(extra[(1, 3)]) == [1, 2, 4]    # upper left, upper, left
    assert sorted(extra[(2, 4)]) == []
    assert g.map_base_tile_to_images(0) == {}
    every = g.base_tile_coordinate_to_image_file_map
    assert sorted(every[(1, 1)]) == [0, 1, 3, 4]
    assert g.get_empty_base_tile_coordinates() == set()
    created = sorted((t['y'], t['x']) for i in range(6) for t in g.map_image_to_base_tiles(i))
    assert created == [(r, c) for r in range(3) for c in range(5)]   # each exactly once


# ---- Image methods and PyramidTile vs the reference -----------------------------

def test_image_extract(img):
    a = img["img_a"]
    for k, args in enumerate(img["extract_args"]):
        got = Image(a).extract(*[int(v) for v in args])
        assert type(got) is Image
        assert np.array_equal(got.array, img["extract_%d" % k])


def test_image_insert_merge_join_pad(img):
    a, b, small = img["img_a"], img["img_b"], img["img_small"]
    base = Image(a.copy())
    copy = base.insert(Image(small), 3, 4, inplace=False)
    assert copy is not base and np.array_equal(base.array, a)
    assert np.array_equal(copy.array, img["insert_copy"])
    assert base.insert(Image(small), 33, 41) is base
    assert np.array_equal(base.array, img["insert_inplace"])
    assert np.array_equal(Image(a.copy()).merge(Image(b), "y", 13, inplace=False).array, img["merge_y"])
    assert np.array_equal(Image(a.copy()).merge(Image(b), "x", 21, inplace=False).array, img["merge_x"])
    m = Image(a.copy())
    assert m.merge(Image(b), "x", 21) is m and np.array_equal(m.array, img["merge_x"])
    assert np.array_equal(Image(a).join(Image(b), "y").array, img["join_y"])
    assert np.array_equal(Image(a).join(Image(b), "x").array, img["join_x"])
    for side in ("top", "bottom", "left", "right"):
        got = Image(small).pad_with_background(3, side).array
        assert got.dtype == np.uint8 and np.array_equal(got, img["pad_" + side])
    with pytest.raises(TypeError):
        Image(a).insert(small, 0, 0)


def _raises(expected, fn):
    if expected is None:
        fn()
        return
    kind = {"ValueError": ValueError, "TypeError": TypeError}[expected[0]]
    with pytest.raises(kind) as e:
        fn()
    assert str(e.value) == expected[1]


def test_reference_errors(geo, img):
    a, b, small = img["img_a"], img["img_b"], img["img_small"]
    err = geo["errors"]
    u8 = np.zeros((4, 4), dtype=np.uint8)
    cases = {
        "insert_too_low": lambda: Image(a).insert(Image(small), 34, 0),
        "insert_too_right": lambda: Image(a).insert(Image(small), 0, 42),
        "merge_axis": lambda: Image(a).merge(Image(b), "z", 0),
        "join_axis": lambda: Image(a).join(Image(b), "z"),
        "pad_side": lambda: Image(a).pad_with_background(1, "front"),
        "tile_uint16": lambda: PyramidTile(np.zeros((4, 4), dtype=np.uint16)),
        "tile_not_array": lambda: PyramidTile([[0]]),
        "tile_1d": lambda: PyramidTile(np.zeros(4, dtype=np.uint8)),
        "tile_too_high": lambda: PyramidTile(np.zeros((257, 4), dtype=np.uint8)),
        "tile_too_wide": lambda: PyramidTile(np.zeros((4, 257), dtype=np.uint8)),
        "tile_empty": lambda: PyramidTile(np.zeros((0, 4), dtype=np.uint8)),
        "tile_256": lambda: PyramidTile(np.zeros((256, 256), dtype=np.uint8)),
        "tile_metadata": lambda: PyramidTile(u8, ImageMetadata()),
        "tile_metadata_ok": lambda: PyramidTile(u8, PyramidTileMetadata(1, 2, 3, 4)),
        "background_noise_no_mu": lambda: PyramidTile.create_as_background(add_noise=True),
        "background_noise_no_sigma": lambda: PyramidTile.create_as_background(add_noise=True, mu=3),
        "background_noise": lambda: PyramidTile.create_as_background(add_noise=True, mu=3, sigma=1),
    }
    assert sorted(cases) == sorted(err)
    for name, fn in cases.items():
        _raises(err[name], fn)


def test_create_as_background(img):
    t = PyramidTile.create_as_background()
    assert isinstance(t, PyramidTile) and t.array.dtype == np.uint8
    assert np.array_equal(t.array, img["background"]) and t.dimensions == (256, 256)
    md = PyramidTileMetadata(3, 1, 2, 9)
    assert PyramidTile.create_as_background(metadata=md).metadata is md
    assert (md.z, md.y, md.x, md.channel_layer_id) == (3, 1, 2, 9)


def test_shrink_unsupported_raises_without_a_kernel():
    with pytest.raises(NotImplementedError, match="factor 2 on uint8"):
        Image(np.zeros((8, 8), dtype=np.uint8)).shrink(3)
    with pytest.raises(NotImplementedError, match="factor 2 on uint8"):
        Image(np.zeros((8, 8), dtype=np.uint16)).shrink(2)


# ---- the planner vs the literal loop ---------------------------------------------

@pytest.mark.parametrize("name", lit.CPU_LAYERS)
def test_planner_matches_literal_loop(name):
    g = lit.make_layer(name)
    sites = lit.random_sites(g)
    want, missing = lit.literal_base_level(g, sites)
    table = P.plan_base_tiles(g)
    assert table.dtype == P.hip.TILE_RECT_DTYPE
    assert np.all(np.diff(table["tile"]) >= 0), "the table is sorted by tile"
    rows, cols = g.dimensions[-1]
    got = P.paint_base_tiles(table, sites, rows, cols)
    assert np.array_equal(got, want)
    assert g.get_empty_base_tile_coordinates() == missing
    for r, c in missing:
        assert not got[r, c].any()
    # the layers are not degenerate: most tiles hold pixels
    assert np.count_nonzero(got.reshape(rows * cols, -1).any(axis=1)) == rows * cols - len(missing)


def test_layers_cover_the_insert_rules():
    """The test layers reach all three insert rules, background padding on
    every side and spacer tiles."""
    t = P.plan_base_tiles(lit.make_layer("two_wells"))
    per_tile = np.bincount(t["tile"])
    assert per_tile.max() == 4 and (per_tile == 1).any() and (per_tile == 2).any()
    assert (t["src_x"] % 16 != 0).any() and (t["dst_x"] % 16 != 0).any()
    assert len(lit.make_layer("two_wells").get_empty_base_tile_coordinates()) > 0
    assert np.bincount(P.plan_base_tiles(lit.make_layer("tile_aligned"))["tile"]).max() == 1
    assert len(lit.make_layer("hole").get_empty_base_tile_coordinates()) > 0


def test_refuses_small_sites():
    for size in ((255, 420), (300, 255)):
        g = P.LayerGeometry(size, [(0, 0, 0, (0, 0))], {0: (1, 1)})
        with pytest.raises(ValueError, match="smaller than"):
            P.plan_base_tiles(g)


def test_refuses_other_zoom_factors():
    g = P.LayerGeometry((300, 420), [(0, 0, 0, (0, 0))], {0: (1, 1)}, zoom_factor=3)
    with pytest.raises(ValueError, match="zoom factor"):
        P.plan_base_tiles(g)


def test_refuses_tile_created_twice():
    # two wells 50 px apart: tile column 1 (256..512) holds pixels of both
    sites = [(0, 0, 0, (0, 0)), (1, 0, 0, (0, 420 + 50))]
    g = P.LayerGeometry((300, 420), sites, {0: (1, 1), 1: (1, 1)})
    with pytest.raises(ValueError, match="created by sites 0 and 1"):
        P.plan_base_tiles(g)
    # a hole whose corner is not tile aligned: the site above it and the site
    # to its left both create the tile at the corner
    sites = [(0, y, x, (y * 300, x * 420)) for y in range(3) for x in range(3) if (y, x) != (1, 1)]
    with pytest.raises(ValueError, match="would be created by sites"):
        P.plan_base_tiles(P.LayerGeometry((300, 420), sites, {0: (3, 3)}))


# ---- the odd-side rule -------------------------------------------------------------

def _fraction_half(a):
    """Exact rational area mean, pixel by pixel, rounded half to even."""
    sy, sx = a.shape
    oy, ox = sy // 2, sx // 2
    fy, fx = Fraction(sy, oy), Fraction(sx, ox)

    def overlap(lo, hi, i):
        return max(Fraction(0), min(hi, Fraction(i + 1)) - max(lo, Fraction(i)))

    out = np.zeros((oy, ox), dtype=np.uint8)
    for j in range(oy):
        wy = [overlap(j * fy, (j + 1) * fy, i) for i in range(sy)]
        for k in range(ox):
            wx = [overlap(k * fx, (k + 1) * fx, i) for i in range(sx)]
            total = sum(wy[r] * wx[c] * int(a[r, c]) for r in range(sy) if wy[r]
                        for c in range(sx) if wx[c])
            out[j, k] = round(total / (fy * fx))   # Fraction.__round__: half to even
    return out


@pytest.mark.parametrize("shape", [(3, 5), (257, 4), (3, 3), (2, 3)])
def test_odd_side_area_mean(shape):
    rng = np.random.default_rng(shape[0] * 1000 + shape[1])
    a = rng.integers(0, 256, shape, dtype=np.uint8)
    got = P._area_mean_odd(a)
    assert got.dtype == np.uint8 and got.shape == (shape[0] // 2, shape[1] // 2)
    assert np.array_equal(got, _fraction_half(a))
    assert np.array_equal(got, lit.exact_half(a))
    assert np.array_equal(Image(a).shrink(2, inplace=False).array, got)   # host path, no kernel


def test_odd_side_rounds_half_to_even():
    # 1 x 3 -> weights (1, 1/2) / 1.5 ... use 3 x 2 -> one pixel, mean of six
    a = np.array([[0, 1], [1, 1], [0, 0]], dtype=np.uint8)    # 3 / 6 = 0.5 -> 0
    assert P._area_mean_odd(a)[0, 0] == 0
    a = np.array([[1, 2], [2, 2], [1, 1]], dtype=np.uint8)    # 9 / 6 = 1.5 -> 2
    assert P._area_mean_odd(a)[0, 0] == 2
    a = np.array([[2, 3], [3, 3], [2, 2]], dtype=np.uint8)    # 15 / 6 = 2.5 -> 2
    assert P._area_mean_odd(a)[0, 0] == 2
    with pytest.raises(ValueError):
        P._area_mean_odd(np.zeros((1, 4), dtype=np.uint8))


def test_tile_storage_round_trip():
    from tmlibrary_amd.image import array_to_tiles, tiles_to_array
    a = np.random.default_rng(5).integers(0, 256, (600, 258), dtype=np.uint8)
    tiles, lh, lw = array_to_tiles(a)
    assert tiles.shape == (3, 2, 256, 256) and (lh, lw) == (88, 2)
    assert np.array_equal(tiles[1, 1, :, :2], a[256:512, 256:258]) and not tiles[1, 1, :, 2:].any()
    assert np.array_equal(tiles_to_array(tiles, lh, lw), a)
