"""A literal numpy restatement of the reference's pyramid loops, for the
pyramid tests (CPU and GPU).  It paints whole tiles the way
tmlib/workflow/illuminati/api.py does -- extract, pad, insert, join, shrink --
with numpy arrays and a dict of images, and shares no code with the planner's
rectangle table (tmlibrary_amd/workflow/pyramid.py plan_base_tiles).  The
site-to-tile maps come from ``LayerGeometry`` (pinned on their own by the
geometry goldens)."""
import numpy as np

from tmlibrary_amd.workflow.pyramid import LayerGeometry

T = 256


# ---- layers -----------------------------------------------------------------

def _well(well_id, rows, cols, size, origin=(0, 0), step=None, absent=()):
    step = step or size
    return [(well_id, y, x, (origin[0] + y * step[0], origin[1] + x * step[1]))
            for y in range(rows) for x in range(cols) if (y, x) not in absent]


def make_layer(name):
    """The layers of the issue's test plan."""
    if name == "one_well":          # 2 x 3 sites of 300 x 420 at offset (0, 0)
        return LayerGeometry((300, 420), _well(0, 2, 3, (300, 420)), {0: (2, 3)})
    if name == "two_wells":         # 500 px apart both ways; offsets no multiple of 256 or 16
        sites = (_well(0, 2, 3, (300, 420), (37, 21)) +
                 _well(1, 2, 3, (300, 420), (37 + 600 + 500, 21 + 1260 + 500)))
        return LayerGeometry((300, 420), sites, {0: (2, 3), 1: (2, 3)})
    if name == "tile_aligned":      # no negative offsets, no neighbours
        return LayerGeometry((256, 512), _well(0, 2, 2, (256, 512)), {0: (2, 2)})
    if name == "hole":
        # 3 x 3 well, centre site absent.  Site rows are tile aligned (512):
        # with an unaligned hole corner the site above and the site left of the
        # hole both create the tile at that corner, which the planner refuses
        # (see test_refuses_tile_created_twice); columns stay unaligned (420).
        return LayerGeometry((512, 420), _well(0, 3, 3, (512, 420), absent=((1, 1),)),
                             {0: (3, 3)})
    if name == "displaced":         # site displacements (7, 3): neighbours overlap
        return LayerGeometry((300, 420), _well(0, 2, 3, (300, 420), step=(293, 417)),
                             {0: (2, 3)}, vertical_site_displacement=7,
                             horizontal_site_displacement=3)
    if name == "production_pitch":  # the production row pitch (GPU only)
        return LayerGeometry((2160, 2560), _well(0, 2, 3, (2160, 2560)), {0: (2, 3)})
    raise KeyError(name)


CPU_LAYERS = ("one_well", "two_wells", "tile_aligned", "hole", "displaced")


def random_sites(geometry, seed=1234):
    rng = np.random.default_rng(seed)
    h, w = geometry.image_size
    return rng.integers(0, 256, (len(geometry.sites), h, w), dtype=np.uint8)


# ---- base level: api.py:391-499 with channel.py:680-736 ----------------------

def literal_extract_tile(image, y_offset, x_offset):
    y_end = y_offset + T
    x_end = x_offset + T
    n_top = n_bottom = n_left = n_right = None
    if y_offset < 0:
        n_top = abs(y_offset)
        y_offset = 0
    elif (image.shape[0] - y_offset) < T:
        n_bottom = T - (image.shape[0] - y_offset)
    if x_offset < 0:
        n_left = abs(x_offset)
        x_offset = 0
    elif (image.shape[1] - x_offset) < T:
        n_right = T - (image.shape[1] - x_offset)
    tile = image[y_offset:y_offset + (y_end - y_offset), x_offset:x_offset + (x_end - x_offset)]
    if n_top is not None:
        tile = np.vstack([np.zeros((n_top, tile.shape[1]), np.uint8), tile])
    if n_bottom is not None:
        tile = np.vstack([tile, np.zeros((n_bottom, tile.shape[1]), np.uint8)])
    if n_left is not None:
        tile = np.hstack([np.zeros((tile.shape[0], n_left), np.uint8), tile])
    if n_right is not None:
        tile = np.hstack([tile, np.zeros((tile.shape[0], n_right), np.uint8)])
    return np.array(tile)


def _insert(tile, sub, y_offset, x_offset):
    assert sub.size > 0, "the reference's PyramidTile rejects an empty subtile"
    assert sub.shape[0] + y_offset <= tile.shape[0] and sub.shape[1] + x_offset <= tile.shape[1]
    tile[y_offset:y_offset + sub.shape[0], x_offset:x_offset + sub.shape[1]] = sub


def literal_base_tiles(geometry, sites):
    """{(row, column): 256 x 256 uint8}: every base tile the reference's jobs
    would write, for ``sites`` [n][H][W]."""
    H, W = geometry.image_size
    created = {}
    for fid, site in enumerate(geometry.sites):
        tiles = geometry.map_image_to_base_tiles(fid)
        image_store = {fid: sites[fid]}
        extra_file_map = geometry.map_base_tile_to_images(fid)
        for t in tiles:
            row, column = t['y'], t['x']
            tile = literal_extract_tile(image_store[fid], t['y_offset'], t['x_offset'])
            file_coordinate = np.array((site.y, site.x))
            for efid in extra_file_map[row, column]:
                if efid not in image_store:
                    image_store[efid] = sites[efid]
                extra = geometry.sites[efid]
                condition = file_coordinate > np.array((extra.y, extra.x))
                pixels = image_store[efid]
                if all(condition):
                    y = H - abs(t['y_offset'])
                    x = W - abs(t['x_offset'])
                    height = abs(t['y_offset'])
                    width = abs(t['x_offset'])
                    _insert(tile, pixels[y:y + height, x:x + width], 0, 0)
                elif condition[0] and not condition[1]:
                    y = H - abs(t['y_offset'])
                    height = abs(t['y_offset'])
                    if t['x_offset'] < 0:
                        x = 0
                        width = tile.shape[1] - abs(t['x_offset'])
                        x_offset = abs(t['x_offset'])
                    else:
                        x = t['x_offset']
                        width = tile.shape[1]
                        x_offset = 0
                    _insert(tile, pixels[y:y + height, x:x + width], 0, x_offset)
                elif not condition[0] and condition[1]:
                    x = W - abs(t['x_offset'])
                    width = abs(t['x_offset'])
                    if t['y_offset'] < 0:
                        y = 0
                        height = tile.shape[0] - abs(t['y_offset'])
                        y_offset = abs(t['y_offset'])
                    else:
                        y = t['y_offset']
                        height = tile.shape[0]
                        y_offset = 0
                    _insert(tile, pixels[y:y + height, x:x + width], y_offset, 0)
                else:
                    raise IndexError('Tile shouldn\'t be in this batch!')
            assert tile.shape == (T, T)
            assert (row, column) not in created, "tile written twice"
            created[(row, column)] = tile
    return created


def literal_base_level(geometry, sites):
    """The base level as [rows][cols][256][256], missing tiles as background
    (api.py:550), and the set of coordinates that were missing."""
    rows, cols = geometry.dimensions[-1]
    created = literal_base_tiles(geometry, sites)
    level = np.zeros((rows, cols, T, T), dtype=np.uint8)
    for (r, c), tile in created.items():
        level[r, c] = tile
    missing = set((r, c) for r in range(rows) for c in range(cols)) - set(created)
    return level, missing


# ---- lower levels: api.py:513-568 --------------------------------------------

def shrink_even(a):
    """(a + b + c + d + 2) >> 2 over 2 x 2 blocks."""
    w = a.astype(np.uint32)
    return ((w[0::2, 0::2] + w[0::2, 1::2] + w[1::2, 0::2] + w[1::2, 1::2] + 2) >> 2).astype(np.uint8)


def exact_half(a):
    """The exact area mean over floor(side / 2) pixels per axis, half to even:
    every input pixel repeated n_out times along an axis, summed in runs of
    n_in (not the weight matrices of the module under test)."""
    sy, sx = a.shape
    oy, ox = sy // 2, sx // 2
    # axis by axis (the sums separate): [sy * oy][sx] -> [oy][sx] -> [oy][sx * ox] -> [oy][ox]
    w = np.repeat(a.astype(np.int64), oy, axis=0).reshape(oy, sy, sx).sum(axis=1)
    num = np.repeat(w, ox, axis=1).reshape(oy, ox, sx).sum(axis=2)
    den = sy * sx
    q, r = np.divmod(num, den)
    up = (2 * r > den) | ((2 * r == den) & (q % 2 == 1))
    return (q + up).astype(np.uint8)


def literal_shrink(mosaic):
    if mosaic.shape[0] % 2 == 0 and mosaic.shape[1] % 2 == 0:
        return shrink_even(mosaic)
    return exact_half(mosaic)


def literal_lower_level(tiles, rows, cols):
    """One level down from a dict {(r, c): array} of a rows x cols level: join
    the existing tiles of (2y..2y+1, 2x..2x+1) along x, then y, and shrink."""
    out = {}
    for y in range((rows + 1) // 2):
        for x in range((cols + 1) // 2):
            pre_rows = [r for r in (2 * y, 2 * y + 1) if r < rows]
            pre_cols = [c for c in (2 * x, 2 * x + 1) if c < cols]
            mosaic_img = None
            for i, r in enumerate(pre_rows):
                row_img = None
                for j, c in enumerate(pre_cols):
                    img = tiles[(r, c)]
                    row_img = img if j == 0 else np.hstack([row_img, img])
                mosaic_img = row_img if i == 0 else np.vstack([mosaic_img, row_img])
            out[(y, x)] = literal_shrink(mosaic_img)
    return out, (rows + 1) // 2, (cols + 1) // 2


def level_to_dict(level, last_h=T, last_w=T):
    rows, cols = level.shape[:2]
    return {(r, c): np.array(level[r, c, :(last_h if r == rows - 1 else T),
                                   :(last_w if c == cols - 1 else T)])
            for r in range(rows) for c in range(cols)}


def dict_to_level(tiles, rows, cols):
    level = np.zeros((rows, cols, T, T), dtype=np.uint8)
    for (r, c), a in tiles.items():
        level[r, c, :a.shape[0], :a.shape[1]] = a
    return level
