"""The illuminati tile pyramid, built on the device from the chain's uint8 sites.

illuminati's product is the zoomable pyramid of 256 x 256 tiles of a channel
layer.  The reference builds it in two steps
(tmlib/workflow/illuminati/api.py):

* ``_create_maxzoom_level_tiles`` (:356-501) stitches every site image into
  base tiles, with pixels from the upper and left neighbouring sites;
* ``_create_lower_zoom_level_tiles`` (:503-573) halves each level: a 2 x 2
  tile mosaic followed by ``Image.shrink``.

Here ``LayerGeometry`` restates the geometry of ``tmlib/models/channel.py``
over plain data (no ORM rows), ``plan_base_tiles`` turns the reference's
per-site loop into one flat table of rectangles, and ``build_pyramid`` runs
the two device passes (``tmh_tiles_base_device``,
``tmh_pyramid_shrink2_device``) over sites that are already resident.
``Pyramid.encode_level`` / ``Pyramid.iter_jpeg_tiles`` then code the tiles as
the JPEG files the reference stores in ``ChannelLayerTile.pixels``
(tmlib/models/tile.py:107-122), a level per call
(``tmh_jpeg_encode_level_device``).  With ``jpeg_quality`` the pyramid is the one
the reference stores: it reads each level back through the JPEG decoder
(``ChannelLayerTile.pixels``, tmlib/models/tile.py:97-105) before halving it,
so every level below the base is built from the JPEG round trip of the level
above (``tmh_jpeg_roundtrip_level_device``).  ``decode_jpeg_tiles`` /
``EncodedLevel.decode`` read stored files back (``tmh_jpeg_decode_tiles``).

Everything in this module except ``build_pyramid`` / ``Pyramid`` is host-only
numpy and needs no device.
"""
from __future__ import annotations

import collections
import contextlib
import ctypes as C
import itertools

import numpy as np

from .. import hip
from ..image import JPEG_STATUS, PyramidTile, decode_jpeg_blob, tiles_to_array
from ..metadata import PyramidTileMetadata

TILE_SIZE = 256

#: one site of a layer, in the order of the image stack: its well, its (y, x)
#: grid position in the well, and ``Site.offset`` (tmlib/models/site.py:135-159)
#: -- the (y, x) pixel position of its top left corner in the layer
Site = collections.namedtuple("Site", ["well_id", "y", "x", "offset"])


class LayerGeometry(object):
    """The geometry of a ``ChannelLayer`` (tmlib/models/channel.py) over plain
    data.  An "image file" of the reference is the index of a site in
    ``sites``; a site without an image is simply absent from the list.

    ``image_size``: (H, W) of every site; ``sites``: ``Site`` tuples (or
    ``(well_id, y, x, (oy, ox))``); ``well_dimensions[well_id] = (rows,
    cols)`` of the well's site grid; the two displacements and the zoom
    factor are the experiment's (``zoom_factor`` must be 2).  ``layer_size``:
    the experiment's ``(pyramid_height, pyramid_width)``; by default the
    extent the sites reach."""

    def __init__(self, image_size, sites, well_dimensions, vertical_site_displacement=0,
                 horizontal_site_displacement=0, zoom_factor=2, layer_size=None):
        self.image_size = (int(image_size[0]), int(image_size[1]))
        self.sites = [Site(s[0], int(s[1]), int(s[2]), (int(s[3][0]), int(s[3][1])))
                      for s in sites]
        if not self.sites:
            raise ValueError("a layer needs at least one site")
        self.well_dimensions = {k: (int(v[0]), int(v[1])) for k, v in well_dimensions.items()}
        self.vertical_site_displacement = int(vertical_site_displacement)
        self.horizontal_site_displacement = int(horizontal_site_displacement)
        self.zoom_factor = zoom_factor
        self._index = {}
        for i, s in enumerate(self.sites):
            if s.well_id not in self.well_dimensions:
                raise ValueError("site %d names a well without dimensions" % i)
            if (s.well_id, s.y, s.x) in self._index:
                raise ValueError("two sites at the same well position")
            if s.offset[0] < 0 or s.offset[1] < 0:
                raise ValueError("site offsets must not be negative")
            self._index[(s.well_id, s.y, s.x)] = i
        if layer_size is None:
            layer_size = (max(s.offset[0] for s in self.sites) + self.image_size[0],
                          max(s.offset[1] for s in self.sites) + self.image_size[1])
        self.height, self.width = int(layer_size[0]), int(layer_size[1])
        self._dimensions = None
        self._tile_map = None

    # ---- channel.py:251-289 ------------------------------------------------
    @property
    def tile_size(self):
        return TILE_SIZE

    @property
    def depth(self):
        return len(self._get_image_sizes(self.height, self.width))

    @property
    def maxzoom_level_index(self):
        return self.depth - 1

    @property
    def n_tiles(self):
        return int(np.sum([np.prod(dims) for dims in self.dimensions]))

    @property
    def dimensions(self):
        """channel.py:273-289: (tile rows, tile columns) of every level, the
        lowest resolution first."""
        if self._dimensions is None:
            levels = list()
            for height, width in self._get_image_sizes(self.height, self.width):
                n_rows = int(np.ceil(float(height) / float(self.tile_size)))
                n_cols = int(np.ceil(float(width) / float(self.tile_size)))
                levels.append((n_rows, n_cols))
            self._dimensions = levels
        return self._dimensions

    def _get_image_sizes(self, height, width):
        """channel.py:343-363: (height, width) of every level, lowest first."""
        levels = list()
        levels.append((height, width))
        while True:
            height = int(np.ceil(float(height) / self.zoom_factor))
            width = int(np.ceil(float(width) / self.zoom_factor))
            levels.append((height, width))
            if height <= self.tile_size and width <= self.tile_size:
                break
        return list(reversed(levels))

    def _calc_tile_indices_and_offsets(self, position, length, displacement):
        """channel.py:365-411.  (The reference's ``else end_offset`` can never
        be taken -- ``i`` runs over ``len(indices)`` -- and is not restated.)"""
        start_fraction = float(position) / float(self.tile_size)
        start_index = int(np.floor(start_fraction))
        start_diff = start_index - start_fraction
        start_offset = int(self.tile_size * start_diff)

        end_fraction = float(position + length - displacement) / float(self.tile_size)
        end_index = int(np.ceil(end_fraction))

        indices = list(range(start_index, end_index))
        return {
            'indices': indices,
            'offsets': [start_offset + i * self.tile_size for i in range(len(indices))]
        }

    def _calc_tile_indices(self, position, length, displacement):
        """channel.py:522-555."""
        start_fraction = float(position) / float(self.tile_size)
        start_index = int(np.floor(start_fraction))
        end_fraction = float(position + length - displacement) / float(self.tile_size)
        end_index = int(np.ceil(end_fraction))
        return list(range(start_index, end_index))

    def _site_tile_indices(self, site):
        rows = self._calc_tile_indices(site.offset[0], self.image_size[0],
                                       self.vertical_site_displacement)
        cols = self._calc_tile_indices(site.offset[1], self.image_size[1],
                                       self.horizontal_site_displacement)
        return rows, cols

    def map_image_to_base_tiles(self, image_file):
        """channel.py:413-503: the base tiles site ``image_file`` creates, each
        with its offset relative to the site.  A tile that overhangs below /
        to the right is left to the neighbour there, when the same well has
        one and the tile is on no well or plate border."""
        mappings = list()
        site = self.sites[image_file]
        well_dimensions = self.well_dimensions[site.well_id]
        y_offset_site, x_offset_site = site.offset
        row_info = self._calc_tile_indices_and_offsets(
            y_offset_site, self.image_size[0], self.vertical_site_displacement)
        col_info = self._calc_tile_indices_and_offsets(
            x_offset_site, self.image_size[1], self.horizontal_site_displacement)
        has_lower_neighbor = (site.well_id, site.y + 1, site.x) in self._index
        has_right_neighbor = (site.well_id, site.y, site.x + 1) in self._index
        for i, y in enumerate(row_info['indices']):
            y_offset = row_info['offsets'][i]
            is_overhanging_vertically = (y_offset + self.tile_size) > self.image_size[0]
            is_not_lower_plate_border = (y + 1) != self.dimensions[-1][0]
            is_not_lower_well_border = (site.y + 1) != well_dimensions[0]
            if is_overhanging_vertically and has_lower_neighbor:
                if is_not_lower_plate_border and is_not_lower_well_border:
                    continue
            for j, x in enumerate(col_info['indices']):
                x_offset = col_info['offsets'][j]
                is_overhanging_horizontally = (x_offset + self.tile_size) > self.image_size[1]
                is_not_right_plate_border = (x + 1) != self.dimensions[-1][1]
                is_not_right_well_border = (site.x + 1) != well_dimensions[1]
                if is_overhanging_horizontally and has_right_neighbor:
                    if is_not_right_plate_border and is_not_right_well_border:
                        continue
                mappings.append({'y': y, 'x': x, 'y_offset': y_offset, 'x_offset': x_offset})
        return mappings

    def map_base_tile_to_images(self, site):
        """channel.py:557-608: for the site with index ``site``, base tile
        (y, x) -> the sites of the same well bordering it above and / or to
        the left whose tile range holds that tile."""
        this = self.sites[site]
        mapping = collections.defaultdict(list)
        for y, x in itertools.product([this.y - 1, this.y], [this.x - 1, this.x]):
            if y == this.y and x == this.x:
                continue
            fid = self._index.get((this.well_id, y, x))
            if fid is None:
                continue
            row_indices, col_indices = self._site_tile_indices(self.sites[fid])
            for ty, tx in itertools.product(row_indices, col_indices):
                mapping[(ty, tx)].append(fid)
        return mapping

    @property
    def base_tile_coordinate_to_image_file_map(self):
        """channel.py:610-644: base tile (y, x) -> every site intersecting it."""
        if self._tile_map is None:
            mapping = collections.defaultdict(list)
            for fid, site in enumerate(self.sites):
                row_indices, col_indices = self._site_tile_indices(site)
                for y, x in itertools.product(row_indices, col_indices):
                    mapping[(y, x)].append(fid)
            self._tile_map = mapping
        return self._tile_map

    def get_empty_base_tile_coordinates(self):
        """channel.py:505-520: base tiles no site maps to (spacers)."""
        tile_coords = self.base_tile_coordinate_to_image_file_map.keys()
        rows = range(self.dimensions[-1][0])
        cols = range(self.dimensions[-1][1])
        all_tile_coords = list(itertools.product(rows, cols))
        return set(all_tile_coords) - set(tile_coords)

    def calc_coordinates_of_next_higher_level(self, z, y, x):
        """channel.py:646-678."""
        coordinates = list()
        max_row, max_column = self.dimensions[z + 1]
        rows = range(y * self.zoom_factor, (y * self.zoom_factor + self.zoom_factor - 1) + 1)
        cols = range(x * self.zoom_factor, (x * self.zoom_factor + self.zoom_factor - 1) + 1)
        for r, c in itertools.product(rows, cols):
            if r < max_row and c < max_column:
                coordinates.append((r, c))
        return coordinates

    def extract_tile_from_image(self, image, y_offset, x_offset):
        """channel.py:680-736: the tile at (y_offset, x_offset) of ``image``,
        zero padded where it leaves the image (host numpy)."""
        y_end = y_offset + self.tile_size
        x_end = x_offset + self.tile_size

        n_top = None
        n_bottom = None
        n_left = None
        n_right = None
        if y_offset < 0:
            n_top = abs(y_offset)
            y_offset = 0
        elif (image.dimensions[0] - y_offset) < self.tile_size:
            n_bottom = self.tile_size - (image.dimensions[0] - y_offset)
        if x_offset < 0:
            n_left = abs(x_offset)
            x_offset = 0
        elif (image.dimensions[1] - x_offset) < self.tile_size:
            n_right = self.tile_size - (image.dimensions[1] - x_offset)

        extracted_pixels = image.extract(
            y_offset, y_end - y_offset, x_offset, x_end - x_offset).array
        tile = PyramidTile(extracted_pixels)
        if n_top is not None:
            tile = tile.pad_with_background(n_top, 'top')
        if n_bottom is not None:
            tile = tile.pad_with_background(n_bottom, 'bottom')
        if n_left is not None:
            tile = tile.pad_with_background(n_left, 'left')
        if n_right is not None:
            tile = tile.pad_with_background(n_right, 'right')
        return tile


# ---------------------------------------------------------------------------
# the planner: api.py:391-499 as a table of rectangles
# ---------------------------------------------------------------------------

_TILE_ERROR = ('Height and width of image must be greater than zero and '
               'maximally %d pixels.' % TILE_SIZE)


def _clip_extract(y, height, x, width, H, W):
    """numpy's ``a[y:y+height, x:x+width]`` of an H x W array (non-negative
    starts): (y, rows, x, cols) after the slices are clipped at the edge."""
    rows = max(0, min(y + height, H) - min(y, H))
    cols = max(0, min(x + width, W) - min(x, W))
    return y, rows, x, cols


def _check_disjoint(rects):
    for a, b in itertools.combinations(rects, 2):
        # (tile, site, src_y, src_x, dst_y, dst_x, height, width)
        if (a[4] < b[4] + b[6] and b[4] < a[4] + a[6] and
                a[5] < b[5] + b[7] and b[5] < a[5] + a[7]):
            raise AssertionError("rectangles of one tile overlap: %r %r" % (a, b))


def plan_base_tiles(geometry):
    """The rectangle table of the base level: a ``hip.TILE_RECT_DTYPE`` array
    of (tile, site, src_y, src_x, dst_y, dst_x, height, width), sorted by
    tile (row-major tile index over ``geometry.dimensions[-1]``).

    Per site and tile it applies, as the reference's loop does: the extract
    and zero padding of ``extract_tile_from_image`` (channel.py:680-736), and
    the three insert rules for pixels of the top left, top and left
    neighbours (api.py:443-490) with their ``abs(offset)`` arithmetic and
    numpy's clipping of slices at the image edge.  Bytes no rectangle covers
    are background (0).

    Raises ``ValueError`` instead of guessing: for sites smaller than a tile
    (a tile could span more sites than the reference's neighbour search
    sees), a zoom factor other than 2, and a base tile two sites would
    create (the reference would write it twice; wells less than a tile
    apart, or a hole in a well grid whose corner is not tile aligned)."""
    g = geometry
    H, W = g.image_size
    T = g.tile_size
    if g.zoom_factor != 2:
        raise ValueError("only a zoom factor of 2 is supported (got %r)" % (g.zoom_factor,))
    if H < T or W < T:
        raise ValueError("sites of %d x %d pixels are smaller than a %d pixel tile" % (H, W, T))
    n_rows, n_cols = g.dimensions[-1]
    owner = {}
    out = []
    for fid, site in enumerate(g.sites):
        tiles = g.map_image_to_base_tiles(fid)
        extra_file_map = g.map_base_tile_to_images(fid)
        for t in tiles:
            row, column = t['y'], t['x']
            if not (0 <= row < n_rows and 0 <= column < n_cols):
                raise ValueError("site %d reaches tile (%d, %d) outside the layer's %d x %d tiles"
                                 % (fid, row, column, n_rows, n_cols))
            if (row, column) in owner:
                raise ValueError("base tile (%d, %d) would be created by sites %d and %d"
                                 % (row, column, owner[(row, column)], fid))
            owner[(row, column)] = fid
            tile_index = row * n_cols + column
            yo, xo = t['y_offset'], t['x_offset']
            rects = []
            # extract_tile_from_image: extract, then pad top / bottom / left / right
            n_top = abs(yo) if yo < 0 else 0
            n_left = abs(xo) if xo < 0 else 0
            y0, x0 = max(yo, 0), max(xo, 0)
            y, h, x, w = _clip_extract(y0, yo + T - y0, x0, xo + T - x0, H, W)
            if h == 0 or w == 0:
                raise ValueError(_TILE_ERROR)
            rects.append((tile_index, fid, y, x, n_top, n_left, h, w))
            for efid in extra_file_map[row, column]:
                extra = g.sites[efid]
                condition = (site.y > extra.y, site.x > extra.x)
                if all(condition):  # pixels from the top left image
                    y, x = H - abs(yo), W - abs(xo)
                    height, width = abs(yo), abs(xo)
                    dst_y, dst_x = 0, 0
                elif condition[0] and not condition[1]:  # from the top image
                    y, height = H - abs(yo), abs(yo)
                    if xo < 0:
                        x, width, dst_x = 0, T - abs(xo), abs(xo)
                    else:
                        x, width, dst_x = xo, T, 0
                    dst_y = 0
                elif not condition[0] and condition[1]:  # from the left image
                    x, width = W - abs(xo), abs(xo)
                    if yo < 0:
                        y, height, dst_y = 0, T - abs(yo), abs(yo)
                    else:
                        y, height, dst_y = yo, T, 0
                    dst_x = 0
                else:
                    raise IndexError('Tile shouldn\'t be in this batch!')
                y, h, x, w = _clip_extract(y, height, x, width, H, W)
                if h == 0 or w == 0:  # PyramidTile(subtile) raises
                    raise ValueError(_TILE_ERROR)
                if h + dst_y > T or w + dst_x > T:
                    raise ValueError('Image doesn\'t fit.')
                rects.append((tile_index, efid, y, x, dst_y, dst_x, h, w))
            _check_disjoint(rects)
            out.extend(rects)
    out.sort(key=lambda r: r[0])
    table = np.zeros(len(out), dtype=hip.TILE_RECT_DTYPE)
    for k, name in enumerate(hip.TILE_RECT_DTYPE.names):
        table[name] = [r[k] for r in out]
    return table


def paint_base_tiles(table, sites, tile_rows, tile_cols):
    """The gather on the host (numpy; tests and documentation -- the product
    path is ``tmh_tiles_base_device``): [tile_rows][tile_cols][256][256]."""
    tiles = np.zeros((tile_rows * tile_cols, TILE_SIZE, TILE_SIZE), dtype=np.uint8)
    for r in table:
        tiles[r["tile"], r["dst_y"]:r["dst_y"] + r["height"], r["dst_x"]:r["dst_x"] + r["width"]] = \
            sites[r["site"], r["src_y"]:r["src_y"] + r["height"], r["src_x"]:r["src_x"] + r["width"]]
    return tiles.reshape(tile_rows, tile_cols, TILE_SIZE, TILE_SIZE)


# ---------------------------------------------------------------------------
# odd mosaics
# ---------------------------------------------------------------------------

def _overlap_weights(n_in, n_out):
    """[n_out][n_in] integer weights: the length, in units of 1 / n_out input
    pixels, that output pixel j's span [j n_in, (j+1) n_in) shares with input
    pixel i's [i n_out, (i+1) n_out).  Every row sums to n_in."""
    j = np.arange(n_out, dtype=np.int64)[:, None]
    i = np.arange(n_in, dtype=np.int64)[None, :]
    lo = np.maximum(j * n_in, i * n_out)
    hi = np.minimum((j + 1) * n_in, (i + 1) * n_out)
    return np.maximum(hi - lo, 0)


def _area_mean_odd(array):
    """Halve an array that has an odd side (no scale-2 integer path exists):
    the exact area mean over floor(side / 2) output pixels per axis, each
    covering side / floor(side / 2) input pixels, rounded half to even, in
    integer arithmetic."""
    a = np.asarray(array)
    sy, sx = a.shape
    oy, ox = sy // 2, sx // 2
    if oy == 0 or ox == 0:
        raise ValueError("an array of %d x %d pixels has no half" % (sy, sx))
    num = _overlap_weights(sy, oy) @ a.astype(np.int64) @ _overlap_weights(sx, ox).T
    den = sy * sx
    q, r = np.divmod(num, den)
    q = q + ((2 * r > den) | ((2 * r == den) & (q % 2 == 1)))
    return q.astype(a.dtype)


# ---------------------------------------------------------------------------
# the device pyramid
# ---------------------------------------------------------------------------

def _device_pointer(x):
    """The device address of ``x`` (an int, a ctypes pointer or anything with
    ``data_ptr()``), or None for a host array."""
    if isinstance(x, np.ndarray):
        return None
    if isinstance(x, C.c_void_p):
        return x.value
    if isinstance(x, int):
        return x
    if hasattr(x, "data_ptr"):
        if not getattr(x, "is_cuda", True) or not x.is_contiguous():
            raise ValueError("a tensor of sites must be a contiguous device tensor")
        return int(x.data_ptr())
    raise TypeError("sites_u8 must be a uint8 numpy array or a device pointer")


class EncodedLevel(object):
    """The JPEG files of one level: ``blob`` (1-D uint8, host) holds them back
    to back in row-major tile order, tile (y, x)'s at ``offsets[y * cols + x]
    : offsets[y * cols + x + 1]`` (int64, tiles + 1 entries); ``dimensions``:
    the level's (tile rows, tile columns)."""

    def __init__(self, blob, offsets, dimensions):
        self.blob = blob
        self.offsets = offsets
        self.dimensions = (int(dimensions[0]), int(dimensions[1]))

    def tile(self, y, x):
        """The file of tile (y, x) as ``bytes``."""
        rows, cols = self.dimensions
        if not (0 <= y < rows and 0 <= x < cols):
            raise IndexError("tile (%d, %d) outside the level's %d x %d tiles" % (y, x, rows, cols))
        t = y * cols + x
        return self.blob[self.offsets[t]:self.offsets[t + 1]].tobytes()

    def __len__(self):
        return self.dimensions[0] * self.dimensions[1]

    def decode(self):
        """The level decoded from its files, stitched into one array as
        ``Pyramid.level`` returns it (on a stored pyramid:
        ``Pyramid.decoded_level``).  Raises ``ValueError`` for a file the
        decoder does not take, or sizes that are no level's."""
        rows, cols = self.dimensions
        tiles, dims, status = decode_jpeg_blob(self.blob, self.offsets)
        _raise_for_status(status)
        dims = dims.reshape(rows, cols, 2)
        last_h, last_w = int(dims[-1, -1, 0]), int(dims[-1, -1, 1])
        want_h = np.where(np.arange(rows) == rows - 1, last_h, TILE_SIZE)[:, None]
        want_w = np.where(np.arange(cols) == cols - 1, last_w, TILE_SIZE)[None, :]
        if np.any(dims[..., 0] != want_h) or np.any(dims[..., 1] != want_w):
            raise ValueError("the files' sizes are not those of one level")
        return tiles_to_array(tiles.reshape(rows, cols, TILE_SIZE, TILE_SIZE), last_h, last_w)


def _raise_for_status(status):
    bad = np.flatnonzero(status)
    if len(bad):
        raise ValueError("JPEG file %d is %s (status %d)"
                         % (bad[0], JPEG_STATUS.get(int(status[bad[0]]), "not decoded"),
                            status[bad[0]]))


def decode_jpeg_tiles(files):
    """The pictures of JPEG files (``bytes`` or uint8 arrays, as
    ``EncodedLevel.tile`` / ``iter_jpeg_tiles`` / ``PyramidTile.jpeg_encode``
    give them), decoded on the device in one call: a list of ``h x w`` uint8
    arrays, the pixels libjpeg decodes.  Raises ``ValueError`` naming the
    first file that is not decoded and its status (1: a JPEG outside what
    libjpeg writes for 8-bit grayscale tiles, 2: corrupt)."""
    parts = [np.frombuffer(f, np.uint8) if isinstance(f, (bytes, bytearray, memoryview))
             else np.ascontiguousarray(f, dtype=np.uint8).ravel() for f in files]
    if not parts:
        return []
    offsets = np.concatenate([[0], np.cumsum([p.size for p in parts])]).astype(np.int64)
    tiles, dims, status = decode_jpeg_blob(np.concatenate(parts), offsets)
    _raise_for_status(status)
    return [np.ascontiguousarray(tiles[t, :dims[t, 0], :dims[t, 1]]) for t in range(len(parts))]


class Pyramid(object):
    """All levels of a layer's pyramid, resident on the device until
    ``close()`` (about 4/3 x 64 KB per base tile).  Level ``z`` is
    ``dimensions[z]`` tiles, level 0 the single top tile, level ``depth - 1``
    the base.  ``jpeg_quality``: None, or the quality of the stored pyramid
    (``build_pyramid``): every level below the base was halved from the JPEG
    round trip of the level above at that quality."""

    def __init__(self, geometry, jpeg_quality=None):
        self.geometry = geometry
        self.jpeg_quality = None if jpeg_quality is None else int(jpeg_quality)
        self.depth = geometry.depth
        self.dimensions = list(geometry.dimensions)
        self.empty_base_tiles = geometry.get_empty_base_tile_coordinates()
        self._closed = False
        self._levels = [None] * self.depth     # hip.DeviceBuffer
        self._last = [None] * self.depth       # (height, width) of the last tile row / column

    def _alloc(self, z):
        rows, cols = self.dimensions[z]
        self._levels[z] = hip.DeviceBuffer(rows * cols * TILE_SIZE * TILE_SIZE)
        return self._levels[z]

    def _check(self, z, y=0, x=0):
        if self._closed:
            raise ValueError("the pyramid is closed")
        if not 0 <= z < self.depth:
            raise IndexError("zoom level %d out of range" % z)
        rows, cols = self.dimensions[z]
        if not (0 <= y < rows and 0 <= x < cols):
            raise IndexError("tile (%d, %d) outside level %d's %d x %d tiles" % (y, x, z, rows, cols))

    def tile_dimensions(self, z, y, x):
        """(height, width) of tile (y, x) of level z: 256 except in the
        level's last row / column."""
        self._check(z, y, x)
        rows, cols = self.dimensions[z]
        return (self._last[z][0] if y == rows - 1 else TILE_SIZE,
                self._last[z][1] if x == cols - 1 else TILE_SIZE)

    def _read_tiles(self, z, first, count):
        return self._levels[z].get((count, TILE_SIZE, TILE_SIZE), np.uint8,
                                   first * TILE_SIZE * TILE_SIZE)

    def tile(self, z, y, x):
        """Tile (y, x) of level z as a ``PyramidTile`` of its ragged size."""
        h, w = self.tile_dimensions(z, y, x)
        full = self._read_tiles(z, y * self.dimensions[z][1] + x, 1)[0]
        return PyramidTile(np.ascontiguousarray(full[:h, :w]), PyramidTileMetadata(z, y, x, None))

    def level(self, z):
        """Level z stitched into one array."""
        self._check(z)
        rows, cols = self.dimensions[z]
        tiles = self._read_tiles(z, 0, rows * cols).reshape(rows, cols, TILE_SIZE, TILE_SIZE)
        return tiles_to_array(tiles, self._last[z][0], self._last[z][1])

    def device_level(self, z):
        """(device pointer, tile rows, tile columns, last row's height, last
        column's width) of level z's tile-major storage."""
        self._check(z)
        return (self._levels[z].ptr,) + tuple(self.dimensions[z]) + tuple(self._last[z])

    def _quality(self, quality):
        if quality is None:
            return 95 if self.jpeg_quality is None else self.jpeg_quality
        if self.jpeg_quality is not None and int(quality) != self.jpeg_quality:
            raise ValueError("this pyramid was built from tiles stored at JPEG quality %d, not %d"
                             % (self.jpeg_quality, int(quality)))
        return int(quality)

    def decoded_level(self, z, quality=None, stream=None):
        """Level z as the reference reads it back from its stored files: the
        JPEG round trip of every tile (``tmh_jpeg_roundtrip_level_device``),
        stitched into one array like ``level(z)``."""
        self._check(z)
        quality = self._quality(quality)
        L = hip.lib()
        rows, cols = self.dimensions[z]
        with hip.DeviceBuffer(rows * cols * TILE_SIZE * TILE_SIZE) as out:
            hip.check(L.tmh_jpeg_roundtrip_level_device(*self.device_level(z), quality, out, stream))
            tiles = out.get((rows, cols, TILE_SIZE, TILE_SIZE), np.uint8, stream=stream)
        return tiles_to_array(tiles, self._last[z][0], self._last[z][1])

    def encode_level(self, z, quality=None, stream=None):
        """Every tile of level z as the JPEG file ``PyramidTile.jpeg_encode``
        (tmlib/image.py:1073-1094) returns for it: an ``EncodedLevel``.  One
        measuring call, one allocation of the exact size, one writing call and
        one device-to-host copy of the blob.  ``quality``: by default the
        pyramid's ``jpeg_quality``, or 95 when that is None; on a stored
        pyramid any other quality raises ``ValueError`` (its lower levels
        were built from files of that quality)."""
        self._check(z)
        quality = self._quality(quality)
        L = hip.lib()
        level = self.device_level(z)
        n = level[1] * level[2]
        total = C.c_int64(0)
        with hip.DeviceBuffer((n + 1) * 8) as d_off:
            hip.check(L.tmh_jpeg_encode_level_device(*level, int(quality), None, 0, d_off,
                                                     C.byref(total), stream))
            with hip.DeviceBuffer(total.value) as d_out:
                hip.check(L.tmh_jpeg_encode_level_device(*level, int(quality), d_out, total.value,
                                                         d_off, C.byref(total), stream))
                blob = d_out.get(total.value, np.uint8, stream=stream)
                offsets = d_off.get(n + 1, np.int64, stream=stream)
        return EncodedLevel(blob, offsets, self.dimensions[z])

    def iter_jpeg_tiles(self, quality=None):
        """``(z, y, x, bytes)`` of every tile of every level -- the rows of
        the reference's ``channel_layer_tiles`` table without the layer id --
        the base level first, then upward; row-major within a level.  One
        level is coded at a time, so the host holds one level's blob.
        ``quality``: as for ``encode_level``."""
        quality = self._quality(quality)
        for z in range(self.depth - 1, -1, -1):
            enc = self.encode_level(z, quality)
            rows, cols = enc.dimensions
            for y, x in itertools.product(range(rows), range(cols)):
                yield z, y, x, enc.tile(y, x)

    def close(self):
        self._closed = True
        levels, self._levels = self._levels, [None] * self.depth
        for buf in levels:
            if buf is not None:
                buf.free()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _odd_mosaics_on_host(pyr, z, src=None):
    """Level z's tiles whose mosaic of level z + 1 tiles has an odd side: the
    device pass left them unwritten; the exact area mean on the host.  ``src``:
    the device level the source tiles are read from (default: level z + 1
    itself; the stored pyramid passes its JPEG round trip)."""
    rows, cols = pyr.dimensions[z]
    for y, x in itertools.product(range(rows), range(cols)):
        coords = pyr.geometry.calc_coordinates_of_next_higher_level(z, y, x)
        pre_rows = sorted(set(c[0] for c in coords))
        pre_cols = sorted(set(c[1] for c in coords))
        mh = sum(pyr.tile_dimensions(z + 1, r, pre_cols[0])[0] for r in pre_rows)
        mw = sum(pyr.tile_dimensions(z + 1, pre_rows[0], c)[1] for c in pre_cols)
        if mh % 2 == 0 and mw % 2 == 0:
            continue
        mosaic = np.vstack([np.hstack([_source_tile(pyr, z + 1, r, c, src) for c in pre_cols])
                            for r in pre_rows])
        half = _area_mean_odd(mosaic)
        full = np.zeros((TILE_SIZE, TILE_SIZE), dtype=np.uint8)
        full[:half.shape[0], :half.shape[1]] = half
        pyr._levels[z].put(full, (y * cols + x) * TILE_SIZE * TILE_SIZE)


def _source_tile(pyr, z, y, x, src):
    if src is None:
        return pyr.tile(z, y, x).array
    h, w = pyr.tile_dimensions(z, y, x)
    full = src.get((TILE_SIZE, TILE_SIZE), np.uint8,
                   (y * pyr.dimensions[z][1] + x) * TILE_SIZE * TILE_SIZE)
    return np.ascontiguousarray(full[:h, :w])


def build_pyramid(geometry, sites_u8, table=None, stream=None, jpeg_quality=None):
    """The pyramid of a layer from its uint8 sites (the chain's output,
    ``Corrector.chain_u8`` / ``tmh_correct_chain_u8_device``).

    ``sites_u8``: a host ``[n, H, W]`` uint8 array, or a device pointer (int,
    ``ctypes.c_void_p`` or a device tensor) to that layout -- then nothing of
    the sites crosses to the host.  ``table``: the rectangle table of
    ``plan_base_tiles(geometry)``, when the caller keeps it across layers of
    one geometry (every channel of an experiment).  ``stream``: the
    hipStream_t the sites were produced on (default stream if None).
    ``jpeg_quality``: None halves the uncoded pixels.  An int builds the
    layer the reference stores: level z - 1 is the halving of level z's JPEG
    round trip at that quality (what ``_create_lower_zoom_level_tiles`` reads
    back through ``ChannelLayerTile.pixels``), at every level, while level z
    itself stays the uncoded pixels, so that ``encode_level(z)`` writes the
    stored files.  The round trip goes into one scratch buffer, sized for the
    base level and freed when the top is done: peak device memory is the
    pyramid plus one base level.
    Returns a ``Pyramid``; the call returns when it is complete."""
    L = hip.lib()
    if table is None:
        table = plan_base_tiles(geometry)
    table = np.ascontiguousarray(table, dtype=hip.TILE_RECT_DTYPE)
    n, (H, W) = len(geometry.sites), geometry.image_size
    dev = _device_pointer(sites_u8)
    if dev is None:
        a = np.ascontiguousarray(sites_u8)
        if a.dtype != np.uint8 or a.shape != (n, H, W):
            raise ValueError("sites_u8 must be a uint8 array of shape %r" % ((n, H, W),))
    pyr = Pyramid(geometry, jpeg_quality)
    scratch = None
    temporaries = contextlib.ExitStack()    # the staged sites and the round trip's scratch
    try:
        if dev is None:
            staged = temporaries.enter_context(hip.DeviceBuffer(a.nbytes))
            staged.put(a, stream=stream)
            dev = staged.ptr.value
        z = pyr.depth - 1
        rows, cols = pyr.dimensions[z]
        hip.check(L.tmh_tiles_base_device(C.c_void_p(dev), n, H, W, hip.ptr(table), len(table),
                                          pyr._alloc(z), rows, cols, stream))
        pyr._last[z] = (TILE_SIZE, TILE_SIZE)
        if jpeg_quality is not None and z > 0:
            scratch = temporaries.enter_context(
                hip.DeviceBuffer(rows * cols * TILE_SIZE * TILE_SIZE))
        while z > 0:
            rows, cols = pyr.dimensions[z]
            if pyr.dimensions[z - 1] != ((rows + 1) // 2, (cols + 1) // 2):
                raise ValueError("level %d of %r tiles does not halve into %r"
                                 % (z, (rows, cols), pyr.dimensions[z - 1]))
            lh, lw = C.c_int(), C.c_int()
            src = pyr._levels[z]
            if jpeg_quality is not None:
                hip.check(L.tmh_jpeg_roundtrip_level_device(src, rows, cols, pyr._last[z][0],
                                                            pyr._last[z][1], pyr.jpeg_quality,
                                                            scratch, stream))
                src = scratch
            hip.check(L.tmh_pyramid_shrink2_device(src, rows, cols, pyr._last[z][0],
                                                   pyr._last[z][1], pyr._alloc(z - 1),
                                                   C.byref(lh), C.byref(lw), stream))
            pyr._last[z - 1] = (lh.value, lw.value)
            if pyr._last[z][0] % 2 or pyr._last[z][1] % 2:
                hip.check(L.tmh_synchronize(stream))
                _odd_mosaics_on_host(pyr, z - 1, scratch)
            z -= 1
        hip.check(L.tmh_synchronize(stream))
    except Exception:
        pyr.close()
        raise
    finally:
        temporaries.close()
    return pyr
