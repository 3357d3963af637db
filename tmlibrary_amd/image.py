"""Image classes of the illumination-correction path, computed on MI355X.

Mirrors the hot-path subset of tmlib/image.py:
  ``Image``                (:35-454; array/metadata checks, ``smooth`` :287-311,
                            ``_shift_and_crop`` / ``align`` :345-454)
  ``ChannelImage``         (:455-682; ``_map_to_uint8`` / ``scale`` :493-568,
                            ``clip`` :570-597, ``_correct_illumination`` :599-631,
                            ``correct`` :633-670, ``png_encode`` :672-682)
  ``IllumstatsImage``      (:1097-1136)
  ``IllumstatsContainer``  (:1139-1213; ``smooth`` :1172-1193,
                            ``get_closest_percentile`` :1195-1213)

plus the illuminati post-correct chain (illuminati/api.py:396-405) as one
fused pass, ``Corrector.chain_u8``.

Smoothing, correction, clipping, alignment and scaling run in libtmhip.so
(no CPU fallback); the host only evaluates numpy slice bounds and LUT
parameters.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import hip
from .metadata import ImageMetadata, IllumstatsImageMetadata, PyramidTileMetadata

#: np.log10(1e-10) on this host: the log of a zero pixel in the correction
#: (image.py:624-626 replaces 0 by 10**-10 before the log10)
ZERO_LOG10 = float(np.log10(np.float64(10 ** -10)))


class Image(object):
    """2-D pixel array + optional metadata (tmlib/image.py:35-311)."""

    __slots__ = ("_array", "_metadata")

    def __init__(self, array, metadata=None):
        self.array = array
        self.metadata = metadata

    @property
    def metadata(self):
        return self._metadata

    @metadata.setter
    def metadata(self, value):
        if value is not None and not isinstance(value, ImageMetadata):
            raise TypeError('Argument "metadata" must have type tmlib.metadata.ImageMetadata.')
        self._metadata = value

    @property
    def array(self):
        return self._array

    @array.setter
    def array(self, value):
        if not isinstance(value, np.ndarray):
            raise TypeError('Argument "array" must have type numpy.ndarray.')
        if value.ndim != 2:
            raise ValueError('Argument "array" must be two dimensional.')
        self._array = value

    @property
    def dimensions(self):
        return self.array.shape

    @property
    def dtype(self):
        return self.array.dtype

    @property
    def is_int(self):
        return issubclass(self.array.dtype.type, np.integer)

    @property
    def is_float(self):
        return issubclass(self.array.dtype.type, np.floating)

    @property
    def is_uint(self):
        return issubclass(self.array.dtype.type, np.unsignedinteger)

    @property
    def is_uint8(self):
        return self.array.dtype == np.uint8

    @property
    def is_uint16(self):
        return self.array.dtype == np.uint16

    def align(self, crop=True, inplace=True):
        """Image.align (tmlib/image.py:412-454): shift by the metadata's
        (y_shift, x_shift) and crop, or zero-pad with crop=False (on the GPU)."""
        if self.metadata is None:
            raise AttributeError('Image requires attribute "metadata" for alignment.')
        md = self.metadata
        w, shape = align_window(self.array.shape, md.y_shift, md.x_shift, md.bottom_residue,
                                md.top_residue, md.right_residue, md.left_residue, crop=crop)
        array = align_array(self.array, w, shape)
        if inplace:
            self.metadata.is_aligned = True
            self.array = array
            return self
        new_object = self.__class__(array, self.metadata)
        new_object.metadata.is_aligned = True
        return new_object

    def extract(self, y_offset, height, x_offset, width):
        """image.py:131-153: the rectangle [y_offset : y_offset + height,
        x_offset : x_offset + width] (numpy slicing: clipped at the edge; a
        view, as in the reference)."""
        array = self.array[y_offset:(y_offset + height), x_offset:(x_offset + width)]
        return self.__class__(array, self.metadata)

    def insert(self, image, y_offset, x_offset, inplace=True):
        """image.py:155-189: write ``image``'s pixels at (y_offset, x_offset)."""
        if not isinstance(image, Image):
            raise TypeError('Argument "image" must have type tmlib.image.Image.')
        if (image.dimensions[0] + y_offset > self.dimensions[0] or
                image.dimensions[1] + x_offset > self.dimensions[1]):
            raise ValueError('Image doesn\'t fit.')
        if inplace:
            array = self.array
        else:
            array = self.array.copy()
        height, width = image.dimensions
        array[y_offset:(y_offset + height), x_offset:(x_offset + width)] = image.array
        if inplace:
            return self
        return self.__class__(array, self.metadata)

    def merge(self, image, axis, offset, inplace=True):
        """image.py:191-226: take ``image``'s pixels from ``offset`` on along
        ``axis`` ('y' or 'x')."""
        if not isinstance(image, Image):
            raise TypeError('Argument "image" must have type tmlib.image.Image.')
        if inplace:
            array = self.array
        else:
            array = self.array.copy()
        if axis == 'y':
            array[offset:, :] = image.array[offset:, :]
        elif axis == 'x':
            array[:, offset:] = image.array[:, offset:]
        else:
            raise ValueError('Unknown axis.')
        if inplace:
            return self
        return self.__class__(array, self.metadata)

    def join(self, image, axis):
        """image.py:228-251: stack ``image`` below ('y') or to the right ('x')."""
        if not isinstance(image, Image):
            raise TypeError('Argument "image" must have type tmlib.image.Image.')
        if axis == 'y':
            array = np.vstack([self.array, image.array])
        elif axis == 'x':
            array = np.hstack([self.array, image.array])
        else:
            raise ValueError('Unknown axis.')
        return self.__class__(array, self.metadata)

    def pad_with_background(self, n, side):
        """image.py:253-285: ``n`` rows / columns of zeros on one side."""
        height, width = self.dimensions
        if side == 'top':
            array = np.zeros((n, width), dtype=self.dtype)
            array = np.vstack([array, self.array])
        elif side == 'bottom':
            array = np.zeros((n, width), dtype=self.dtype)
            array = np.vstack([self.array, array])
        elif side == 'left':
            array = np.zeros((height, n), dtype=self.dtype)
            array = np.hstack([array, self.array])
        elif side == 'right':
            array = np.zeros((height, n), dtype=self.dtype)
            array = np.hstack([self.array, array])
        else:
            raise ValueError('Unknown side.')
        return self.__class__(array, self.metadata)

    def shrink(self, factor, inplace=True):
        """image.py:313-343: shrink both axes by ``factor``, each output pixel
        the mean of its neighbourhood (cv2.resize, INTER_AREA, to
        (width / factor, height / factor) with Python 2's integer division).

        Factor 2 on uint8 only (what the pyramid uses): even sides run on the
        device, (a + b + c + d + 2) >> 2 per pixel (OpenCV's integer path at
        scale 2); an array with an odd side has no such path and takes the
        host's exact area mean over floor(side / 2) pixels, rounded half to
        even (workflow/pyramid.py)."""
        if factor != 2 or self.array.dtype != np.uint8:
            raise NotImplementedError(
                'Image.shrink supports factor 2 on uint8 arrays only '
                '(got factor %r on %s).' % (factor, self.array.dtype))
        height, width = self.dimensions
        if height % 2 or width % 2:
            from .workflow.pyramid import _area_mean_odd
            array = _area_mean_odd(self.array)
        else:
            array = shrink2_array(self.array)
        if inplace:
            self.array = array
            return self
        return self.__class__(array, self.metadata)

    def smooth(self, sigma, inplace=True):
        """Gaussian smoothing (image.py:287-311 -> mahotas.gaussian_filter),
        'reflect' border, radius int(4*sigma+0.5), float64, on the GPU."""
        array = smooth_f64(self.array, sigma)
        if inplace:
            self.array = array
            self.metadata.is_smoothed = True
            return self
        new_img = self.__class__(array, self.metadata)
        new_img.metadata.is_smoothed = True
        return new_img


def align_window(shape, y, x, bottom, top, right, left, crop=True):
    """The numpy slicing of tmlib/image.py:345-410 as a tmh_window: the source
    slice ``[top-y : -(bottom+y) or H, left-x : -(right+x) or W]`` and, for
    crop=False, its destination at (top, left).  Returns (window, out_shape);
    raises like the reference when the pasted window does not fit."""
    H, W = int(shape[0]), int(shape[1])
    row_start, row_end = top - y, bottom + y
    row_end = H if row_end == 0 else -row_end
    col_start, col_end = left - x, right + x
    col_end = W if col_end == 0 else -col_end
    rs, re_, _ = slice(row_start, row_end).indices(H)
    cs, ce, _ = slice(col_start, col_end).indices(W)
    rows, cols = max(0, re_ - rs), max(0, ce - cs)
    w = np.zeros((), dtype=hip.WINDOW_DTYPE)
    w["src_r0"], w["src_c0"], w["rows"], w["cols"] = rs, cs, rows, cols
    if crop:
        return w, (rows, cols)
    # aligned_im[top:top+rows, left:left+cols] = extracted (numpy assignment,
    # negative starts included)
    dr = range(H)[top:top + rows]
    dc = range(W)[left:left + cols]
    # numpy broadcasting: equal extents, or a 1-extent source into an empty slice
    ok = all(n == len(t) or (n == 1 and len(t) == 0) for n, t in ((rows, dr), (cols, dc)))
    if not ok:
        raise Exception("Shifting and cropping of the image failed!\n"
                        "Reason: could not broadcast input array from shape (%d,%d) into "
                        "shape (%d,%d)" % (rows, cols, len(dr), len(dc)))
    if len(dr) == 0 or len(dc) == 0:
        w["rows"] = w["cols"] = 0  # nothing pasted
        return w, (H, W)
    w["dst_r0"], w["dst_c0"] = dr.start, dc.start
    return w, (H, W)


def align_array(array: np.ndarray, window, out_shape) -> np.ndarray:
    a = np.ascontiguousarray(array)
    if a.dtype not in (np.uint8, np.uint16):
        raise TypeError("only uint8/uint16 images are aligned on the device")
    out = np.empty(out_shape, dtype=a.dtype)
    win = np.ascontiguousarray(np.asarray(window, dtype=hip.WINDOW_DTYPE).reshape(1))
    hip.check(hip.lib().tmh_align(hip.ptr(a), hip.ptr(out), a.itemsize, 1, a.shape[0],
                                  a.shape[1], hip.ptr(win), out_shape[0], out_shape[1]))
    return out


_TILE = 256


def array_to_tiles(array: np.ndarray):
    """An array cut into tile-major storage [rows][cols][256][256] (ragged
    last row / column zero padded): (tiles, last row's height, last column's
    width)."""
    h, w = array.shape
    rows, cols = -(-h // _TILE), -(-w // _TILE)
    full = np.zeros((rows * _TILE, cols * _TILE), dtype=array.dtype)
    full[:h, :w] = array
    tiles = full.reshape(rows, _TILE, cols, _TILE).transpose(0, 2, 1, 3)
    return np.ascontiguousarray(tiles), h - (rows - 1) * _TILE, w - (cols - 1) * _TILE


def tiles_to_array(tiles: np.ndarray, last_h: int, last_w: int) -> np.ndarray:
    """The inverse of ``array_to_tiles``."""
    rows, cols = tiles.shape[:2]
    full = tiles.transpose(0, 2, 1, 3).reshape(rows * _TILE, cols * _TILE)
    return np.ascontiguousarray(full[:(rows - 1) * _TILE + last_h, :(cols - 1) * _TILE + last_w])


#: status of a file given to the JPEG decoder (tmh_jpeg_decode_tiles)
JPEG_STATUS = {0: "ok", 1: "unsupported", 2: "corrupt"}


def decode_jpeg_blob(blob: np.ndarray, offsets: np.ndarray):
    """JPEG files ``blob[offsets[t]:offsets[t + 1]]`` decoded on the device
    (``tmh_jpeg_decode_tiles``): ``(tiles [n][256][256] uint8 with each
    picture in its corner, dims [n][2] int32, status [n] int32)``."""
    blob = np.ascontiguousarray(blob, dtype=np.uint8)
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    n = len(offsets) - 1
    if n < 0 or (n and offsets[-1] > blob.size):
        raise ValueError("offsets do not fit the blob")
    tiles = np.empty((n, _TILE, _TILE), dtype=np.uint8)
    dims = np.empty((n, 2), dtype=np.int32)
    status = np.empty(n, dtype=np.int32)
    hip.check(hip.lib().tmh_jpeg_decode_tiles(hip.ptr(blob), hip.ptr(offsets), n, hip.ptr(tiles),
                                              hip.ptr(dims), hip.ptr(status)))
    return tiles, dims, status


def shrink2_array(array: np.ndarray) -> np.ndarray:
    """A uint8 array with even sides halved on the device (tmh_pyramid_shrink2)."""
    a = np.ascontiguousarray(array)
    if a.dtype != np.uint8 or a.ndim != 2 or a.shape[0] % 2 or a.shape[1] % 2 or a.size == 0:
        raise ValueError("shrink2_array takes a non-empty uint8 array with even sides")
    tiles, last_h, last_w = array_to_tiles(a)
    rows, cols = tiles.shape[:2]
    out = np.zeros(((rows + 1) // 2, (cols + 1) // 2, _TILE, _TILE), dtype=np.uint8)
    oh, ow = C.c_int(), C.c_int()
    hip.check(hip.lib().tmh_pyramid_shrink2(hip.ptr(tiles), rows, cols, last_h, last_w,
                                            hip.ptr(out), C.byref(oh), C.byref(ow)))
    return tiles_to_array(out, oh.value, ow.value)


def smooth_f64(array: np.ndarray, sigma) -> np.ndarray:
    L = hip.lib()
    a = np.ascontiguousarray(array, dtype=np.float64)
    if a.ndim != 2:
        raise ValueError("smoothing needs a 2-D array")
    out = np.empty_like(a)
    hip.check(L.tmh_smooth_f64(hip.ptr(a), hip.ptr(out), a.shape[0], a.shape[1], float(sigma)))
    return out


class ChannelImage(Image):
    """Grayscale uint8/uint16 site image (tmlib/image.py:455-670)."""

    @staticmethod
    def _map_to_uint8(img, lower_bound=None, upper_bound=None):
        """tmlib/image.py:493-531: uint16 -> uint8 through the reference's numpy
        LUT (evaluated bit-exactly per pixel on the GPU).  Bounds default to the
        image's min / max (the reference's intent; its py3 range check would
        raise on None)."""
        if img.dtype != np.uint16:
            raise TypeError('"img" must have 16-bit unsigned integer type.')
        if lower_bound is not None and not (0 <= lower_bound < 2 ** 16):
            raise ValueError('"lower_bound" must be in the range [0, 65535]')
        if upper_bound is not None and not (0 <= upper_bound < 2 ** 16):
            raise ValueError('"upper_bound" must be in the range [0, 65535]')
        if lower_bound is None:
            lower_bound = np.min(img)
        if upper_bound is None:
            upper_bound = np.max(img)
        if lower_bound >= upper_bound:
            raise ValueError('"lower_bound" must be smaller than "upper_bound"')
        a = np.ascontiguousarray(img)
        out = np.empty(a.shape, dtype=np.uint8)
        hip.check(hip.lib().tmh_map_u16_to_u8(hip.ptr(a), hip.ptr(out), a.size, int(lower_bound),
                                               int(upper_bound)))
        return out

    def scale(self, lower, upper, inplace=True):
        """tmlib/image.py:533-568: map [lower, upper] to [0, 255] (uint16 only;
        uint8 images are returned unchanged)."""
        if self.is_uint16:
            array = self._map_to_uint8(self.array, lower, upper)
            if inplace:
                self.array = array
                self.metadata.is_rescaled = True
                return self
            new_image = self.__class__(array, self.metadata)
            new_image.metadata.is_rescaled = True
            return new_image
        return self

    def __init__(self, array, metadata=None):
        super(ChannelImage, self).__init__(array, metadata)
        if not self.is_uint:
            raise TypeError("Image must have unsigned integer type.")

    @property
    def array(self):
        return self._array

    @array.setter
    def array(self, value):
        if not isinstance(value, np.ndarray):
            raise TypeError('Argument "array" must have type numpy.ndarray.')
        if value.ndim != 2:
            raise ValueError('Argument "array" must be two dimensional.')
        if not (value.dtype == np.uint16 or value.dtype == np.uint8):
            raise ValueError('Argument "array" must have numpy.uint8 or numpy.uint16 data type.')
        self._array = value

    def clip(self, lower, upper, inplace=True):
        """np.clip of the pixels (image.py:570-597), on the GPU."""
        array = clip_array(self.array, lower, upper)
        if inplace:
            self.array = array
            self.metadata.is_clipped = True
            return self
        new_image = self.__class__(array, self.metadata)
        new_image.metadata.is_clipped = True
        return new_image

    @staticmethod
    def _correct_illumination(img, mean, std, log_transform=True):
        """image.py:599-631: log10 -> z-score -> rescale by mean(std),
        mean(mean) -> 10** -> cast to the input dtype (x86 astype rule)."""
        corr = Corrector(mean, std, log_transform=log_transform)
        try:
            return corr.apply(img)
        finally:
            corr.close()

    def correct(self, stats, inplace=True):
        """image.py:633-670: correct with the container's (smoothed) stats."""
        if not isinstance(stats, IllumstatsContainer):
            raise TypeError('Argument "stats" must have type tmlib.image.IllumstatsContainer.')
        if (stats.mean.metadata.channel_id != self.metadata.channel_id or
                stats.std.metadata.channel_id != self.metadata.channel_id):
            raise ValueError("Channels don't match!")
        array = stats.corrector().apply(self.array)
        if inplace:
            self.array = array
            self.metadata.is_corrected = True
            return self
        new_object = ChannelImage(array, self.metadata)
        new_object.metadata.is_corrected = True
        return new_object

    def png_encode(self):
        """image.py:672-682: the image's PNG file as a 1-D uint8 array, coded
        on the device (``tmh_png_encode`` over this one image;
        ``png_encode_sites`` codes many in one call).  A standard greyscale PNG
        of bit depth 8 or 16 that decodes to the pixels; its bytes are not those
        ``cv2.imencode('.png', array)`` gets from libpng."""
        a = self.array
        if not (a.dtype == np.uint8 or a.dtype == np.uint16):
            raise TypeError("Image must have 8-bit or 16-bit unsigned integer type.")
        a = np.ascontiguousarray(a)
        L = hip.lib()
        out = np.empty(int(L.tmh_png_bound(a.shape[0], a.shape[1], a.itemsize)), dtype=np.uint8)
        offsets = np.zeros(2, dtype=np.int64)
        total = C.c_int64(0)
        hip.check(L.tmh_png_encode(hip.ptr(a), 1, a.shape[0], a.shape[1], a.itemsize, hip.ptr(out),
                                   out.nbytes, hip.ptr(offsets), C.byref(total)))
        return out[:total.value].copy()


class EncodedPngs(object):
    """The PNG files of a batch of sites: ``blob`` (1-D uint8, host) holds them
    back to back, site i's at ``offsets[i] : offsets[i + 1]`` (int64, sites + 1
    entries)."""

    def __init__(self, blob, offsets):
        self.blob = blob
        self.offsets = offsets

    def file(self, i):
        """The file of site i as ``bytes``."""
        if not 0 <= i < len(self):
            raise IndexError("file %d of %d" % (i, len(self)))
        return self.blob[self.offsets[i]:self.offsets[i + 1]].tobytes()

    def __len__(self):
        return len(self.offsets) - 1

    def __iter__(self):
        return (self.file(i) for i in range(len(self)))


def png_encode_sites(sites) -> EncodedPngs:
    """The PNG files of ``sites``, [n, H, W] or [H, W] uint8 / uint16, in one
    ``tmh_png_encode_device`` call: a numpy array, or a device tensor (an int16
    tensor is taken as the uint16 bits, as ``DeviceChunkEncoder.deflate`` does)
    -- the uint8 sites ``Corrector.chain_u8`` leaves on the device are coded
    without a host round trip.  No CPU fallback."""
    L = hip.lib()
    src = None
    if isinstance(sites, np.ndarray):
        if not (sites.dtype == np.uint8 or sites.dtype == np.uint16):
            raise TypeError("sites must have 8-bit or 16-bit unsigned integer type.")
        a = np.ascontiguousarray(sites)
        shape, es = a.shape, a.itemsize
    else:
        import torch
        if not isinstance(sites, torch.Tensor) or not sites.is_cuda:
            raise TypeError("sites must be a numpy array or a device tensor")
        if sites.dtype not in (torch.uint8, torch.int16, getattr(torch, "uint16", torch.int16)):
            raise TypeError("sites must have 8-bit or 16-bit unsigned integer type (int16 bits).")
        a = sites.contiguous()
        shape, es = tuple(a.shape), a.element_size()
    if len(shape) == 2:
        shape = (1,) + tuple(shape)
    if len(shape) != 3:
        raise ValueError("sites must be [n, H, W] or [H, W]")
    n, h, w = (int(v) for v in shape)
    if n == 0:
        return EncodedPngs(np.zeros(0, np.uint8), np.zeros(1, np.int64))
    dst_bytes = n * int(L.tmh_png_bound(h, w, es))
    scr_bytes = int(L.tmh_png_scratch_bytes(n, h, w, es))
    if dst_bytes <= 0 or scr_bytes <= 0:
        raise ValueError("sites must have positive height and width")
    try:
        if isinstance(a, np.ndarray):
            src = hip.DeviceBuffer.from_array(a)
            images = src
        else:
            import torch
            torch.cuda.synchronize(a.device)  # the tensor's producers are through
            images = C.c_void_p(a.data_ptr())
        with hip.DeviceBuffer(dst_bytes) as d_dst, hip.DeviceBuffer(scr_bytes) as d_scr, \
                hip.DeviceBuffer(8 * (n + 1)) as d_off:
            hip.check(L.tmh_png_encode_device(images, n, h, w, es, d_dst, dst_bytes, d_off, d_scr,
                                              scr_bytes, None))
            hip.check(L.tmh_synchronize(None))
            offsets = d_off.get((n + 1,), np.int64)
            blob = d_dst.get((int(offsets[n]),), np.uint8)
    finally:
        if src is not None:
            src.free()
    return EncodedPngs(blob, offsets)


def clip_array(array: np.ndarray, lower, upper) -> np.ndarray:
    info = np.iinfo(array.dtype)
    for b in (lower, upper):
        if not (info.min <= int(b) <= info.max):
            raise OverflowError("Python integer %d out of bounds for %s" % (int(b), array.dtype))
    L = hip.lib()
    a = np.ascontiguousarray(array)
    if a.dtype == np.uint8:
        wide = a.astype(np.uint16)
        out = np.empty_like(wide)
        hip.check(L.tmh_clip_u16(hip.ptr(wide), hip.ptr(out), wide.size, int(lower), int(upper)))
        return out.astype(np.uint8)
    out = np.empty_like(a)
    hip.check(L.tmh_clip_u16(hip.ptr(a), hip.ptr(out), a.size, int(lower), int(upper)))
    return out


class Corrector(object):
    """Device-resident correction for one (mean, std) pair.

    Holds tmh_corrector: per-pixel coefficients and the two global means
    (np.mean(std), np.mean(mean), image.py:627) computed once, so a loop of
    ``correct`` calls (illuminati/api.py:389-405) does not redo them.
    """

    def __init__(self, mean, std, log_transform=True):
        L = hip.lib()
        m = np.ascontiguousarray(mean, dtype=np.float64)
        s = np.ascontiguousarray(std, dtype=np.float64)
        if m.shape != s.shape or m.ndim != 2:
            raise ValueError("mean and std must be 2-D arrays of the same shape")
        self.shape = m.shape
        self.log_transform = bool(log_transform)
        h = C.c_void_p()
        hip.check(L.tmh_corrector_create(hip.ptr(m), hip.ptr(s), m.shape[0], m.shape[1],
                                         int(self.log_transform), ZERO_LOG10, C.byref(h)))
        self._h = h

    def means(self):
        a, b = C.c_double(), C.c_double()
        hip.check(hip.lib().tmh_corrector_means(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def apply(self, img: np.ndarray, clip=None, out=None) -> np.ndarray:
        """Correct one image [H,W] or a stack [n,H,W] (uint8/uint16).

        ``out``: optional C-contiguous array of the same shape and dtype to
        write into (a reused buffer skips the first-touch page faults of a
        fresh result, which bound the host path's rate)."""
        img = np.asarray(img)
        if img.shape[-2:] != self.shape:
            raise ValueError("operands could not be broadcast together with shapes %s %s"
                             % (img.shape, self.shape))
        a = np.ascontiguousarray(img)
        if out is None:
            out = np.empty_like(a)
        elif (not isinstance(out, np.ndarray) or out.shape != a.shape or out.dtype != a.dtype
              or not out.flags.c_contiguous or not out.flags.writeable):
            raise ValueError("out must be a writeable C-contiguous %s array of shape %s"
                             % (a.dtype, a.shape))
        elif np.shares_memory(out, a):
            raise ValueError("out must not overlap the input")
        n = 1 if a.ndim == 2 else int(np.prod(a.shape[:-2]))
        lo, hi = (-1, -1) if clip is None else (int(clip[0]), int(clip[1]))
        L = hip.lib()
        if a.dtype == np.uint16:
            hip.check(L.tmh_correct_u16(self._h, hip.ptr(a), hip.ptr(out), n, lo, hi))
        elif a.dtype == np.uint8:
            hip.check(L.tmh_correct_u8(self._h, hip.ptr(a), hip.ptr(out), n, lo, hi))
        else:
            raise TypeError("only uint8/uint16 images can be corrected")
        return out

    def chain_u8(self, sites: np.ndarray, windows, clip_lo: int, clip_hi: int) -> np.ndarray:
        """illuminati/api.py:396-405 for a stack of uint16 sites [n,H,W] in one
        pass: correct -> align(crop=False) with each site's window (see
        ``align_window``) -> clip(clip_lo, clip_hi) -> scale -> uint8."""
        a = np.ascontiguousarray(sites)
        if a.dtype != np.uint16:
            raise TypeError("the chain takes uint16 sites")
        if a.ndim == 2:
            a = a[None]
        if a.shape[-2:] != self.shape:
            raise ValueError("site shape %s does not match the statistics %s"
                             % (a.shape[-2:], self.shape))
        win = np.ascontiguousarray(np.asarray(windows, dtype=hip.WINDOW_DTYPE).reshape(-1))
        if win.size != a.shape[0]:
            raise ValueError("one alignment window per site is required")
        out = np.empty(a.shape, dtype=np.uint8)
        hip.check(hip.lib().tmh_correct_chain_u8(self._h, hip.ptr(a), hip.ptr(out), a.shape[0],
                                                  hip.ptr(win), int(clip_lo), int(clip_hi)))
        return out

    def close(self):
        if getattr(self, "_h", None):
            hip.lib().tmh_corrector_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PyramidTile(Image):
    """A pyramid tile: uint8, at most 256 x 256 pixels (tmlib/image.py:927-1094).
    ``jpeg_encode`` and the JPEG decoders ``create_from_binary`` /
    ``create_from_buffer`` (image.py:993-1037) run on the device."""

    TILE_SIZE = 256

    def __init__(self, array, metadata=None):
        if metadata is not None and not isinstance(metadata, PyramidTileMetadata):
            raise TypeError('Argument "metadata" must have type '
                            'tmlib.metadata.PyramidTileMetadata.')
        super(PyramidTile, self).__init__(array, metadata)
        if not self.is_uint8:
            raise TypeError('Image must have 8-bit unsigned integer data type.')
        if any([d > self.TILE_SIZE or d == 0 for d in self.array.shape]):
            raise ValueError('Height and width of image must be greater than zero and '
                             'maximally %d pixels.' % self.TILE_SIZE)

    @property
    def metadata(self):
        return self._metadata

    @metadata.setter
    def metadata(self, value):
        if value is not None:
            if not isinstance(value, PyramidTileMetadata):
                raise TypeError('Argument "metadata" must have type '
                                'tmlib.metadata.PyramidTileMetadata.')
        self._metadata = value

    @property
    def array(self):
        return self._array

    @array.setter
    def array(self, value):
        if not isinstance(value, np.ndarray):
            raise TypeError('Argument "array" must have type numpy.ndarray.')
        if value.ndim != 2:
            raise ValueError('Argument "array" must be two dimensional.')
        if not value.dtype == np.uint8:
            raise ValueError('Argument "array" must have numpy.uint8 data type.')
        self._array = value

    @classmethod
    def create_as_background(cls, add_noise=False, mu=None, sigma=None, metadata=None):
        """image.py:1039-1071: a tile of zeros.  (With ``add_noise`` the
        reference builds a 1-D array its own constructor then rejects; the
        missing-argument ``ValueError`` comes first and is kept.)"""
        if add_noise:
            if mu is None or sigma is None:
                raise ValueError('Arguments "mu" and "sigma" are required '
                                 'when argument "add_noise" is set to True.')
            array = np.random.normal(mu, sigma, cls.TILE_SIZE ** 2).astype(np.uint8)
        else:
            array = np.zeros((cls.TILE_SIZE,) * 2, dtype=np.uint8)
        return cls(array, metadata)

    @classmethod
    def create_from_binary(cls, string, metadata=None):
        """image.py:993-1014: the tile of a JPEG file given as a binary string
        -- the pixels ``cv2.imdecode`` returns through libjpeg, decoded on the
        device (``tmh_jpeg_decode_tiles`` over this one file;
        ``workflow.pyramid.decode_jpeg_tiles`` decodes many in one call).  A
        file the decoder does not take raises ``ValueError``."""
        return cls.create_from_buffer(string, metadata)

    @classmethod
    def create_from_buffer(cls, buf, metadata=None):
        """image.py:1016-1037: as ``create_from_binary``, from a buffer object."""
        data = np.frombuffer(buf, np.uint8)
        tiles, dims, status = decode_jpeg_blob(data, np.array([0, data.size], dtype=np.int64))
        if status[0]:
            raise ValueError("not a JPEG file this decoder takes: %s"
                             % JPEG_STATUS.get(int(status[0]), status[0]))
        return cls(np.ascontiguousarray(tiles[0, :dims[0, 0], :dims[0, 1]]), metadata)

    def jpeg_encode(self, quality=95):
        """image.py:1073-1094: the tile's JPEG file as a 1-D uint8 array --
        the bytes ``cv2.imencode('.jpeg', array, [cv2.IMWRITE_JPEG_QUALITY,
        quality])`` produces through libjpeg, coded on the device
        (``tmh_jpeg_encode_level`` over a level of this one tile;
        ``Pyramid.encode_level`` codes a whole level in one call)."""
        h, w = self.array.shape
        full = np.zeros((self.TILE_SIZE,) * 2, dtype=np.uint8)
        full[:h, :w] = self.array
        L = hip.lib()
        offsets = np.zeros(2, dtype=np.int64)
        total = C.c_int64(0)
        hip.check(L.tmh_jpeg_encode_level(hip.ptr(full), 1, 1, h, w, int(quality), None, 0,
                                          hip.ptr(offsets), C.byref(total)))
        out = np.empty(total.value, dtype=np.uint8)
        hip.check(L.tmh_jpeg_encode_level(hip.ptr(full), 1, 1, h, w, int(quality), hip.ptr(out),
                                          out.nbytes, hip.ptr(offsets), C.byref(total)))
        return out


def correct_stack(corrector, planes: np.ndarray, site, slot, windows, n_sites: int, slots: int,
                  out_shape) -> np.ndarray:
    """jterator's input loop (jterator/api.py:283-316) for the uint16 planes
    [n, H, W] of one channel in one launch: plane p corrected (``corrector``
    None: not corrected), cropped to its crop=True window and written to slot
    ``slot[p]`` of site ``site[p]``.  Returns [n_sites, out_h, out_w, slots];
    a (site, slot) no plane maps to is 0."""
    a = np.ascontiguousarray(planes)
    if a.dtype != np.uint16 or a.ndim != 3:
        raise TypeError("the stack takes uint16 planes [n, H, W]")
    if corrector is not None and a.shape[-2:] != corrector.shape:
        raise ValueError("operands could not be broadcast together with shapes %s %s"
                         % (a.shape, corrector.shape))
    site = np.ascontiguousarray(site, dtype=np.int32).reshape(-1)
    slot = np.ascontiguousarray(slot, dtype=np.int32).reshape(-1)
    win = np.ascontiguousarray(np.asarray(windows, dtype=hip.WINDOW_DTYPE).reshape(-1))
    if not (site.size == slot.size == win.size == a.shape[0]):
        raise ValueError("one site, slot and alignment window per plane is required")
    oh, ow = int(out_shape[0]), int(out_shape[1])
    out = np.empty((int(n_sites), oh, ow, int(slots)), dtype=np.uint16)
    hip.check(hip.lib().tmh_correct_stack_u16(
        None if corrector is None else corrector._h, hip.ptr(a), hip.ptr(out), a.shape[0],
        a.shape[1], a.shape[2], hip.ptr(site), hip.ptr(slot), hip.ptr(win), int(n_sites),
        int(slots), oh, ow))
    return out


def _int32_planes(planes):
    """the int32 label planes [n, H, W], C-contiguous"""
    a = np.ascontiguousarray(planes)
    if a.dtype != np.int32 or a.ndim != 3:
        raise TypeError("label planes must be an int32 array [n, H, W]")
    return a


def object_tables(planes: np.ndarray) -> np.ndarray:
    """The object tables of int32 label planes [n, H, W] in one call: a
    structured array [n, max_label + 1] of ``hip.OBJECT_ROW_DTYPE`` (pixel
    count, row and column sums, mh.labeled.bbox, border flag per label;
    max_label over all planes).  A negative label raises ValueError."""
    a = _int32_planes(planes)
    L = hip.lib()
    n = a.shape[0]
    if a.size == 0:
        return np.zeros((n, 1), dtype=hip.OBJECT_ROW_DTYPE)
    mx = C.c_int32(0)
    per = 4096  # rows per plane of the first attempt; a larger table is sized from *max_label
    while True:
        rows = np.empty((n, per), dtype=hip.OBJECT_ROW_DTYPE)
        rc = L.tmh_object_table(hip.ptr(a), n, a.shape[1], a.shape[2], C.byref(mx), hip.ptr(rows),
                                rows.size)
        if rc == hip.TMH_EINVAL and mx.value + 1 > per:
            per = mx.value + 1
            continue
        hip.check(rc)
        return rows.reshape(-1)[:n * (mx.value + 1)].reshape(n, mx.value + 1)


def object_contours(planes: np.ndarray):
    """The object tables and every object's borders of int32 label planes
    [n, H, W] in one ``tmh_object_contours`` call: ``(rows, objects, contours,
    points)`` -- rows and objects [n, max_label + 1] of ``hip.OBJECT_ROW_DTYPE``
    and ``hip.CONTOUR_OBJECT_DTYPE``, contours of ``hip.CONTOUR_DTYPE`` in
    (plane, label, discovery) order, points int32 [n_points, 2] as (x, y) of
    each object's padded bounding-box mask.  A negative label raises ValueError."""
    a = _int32_planes(planes)
    L = hip.lib()
    n = a.shape[0]
    if a.size == 0:
        return (np.zeros((n, 1), dtype=hip.OBJECT_ROW_DTYPE),
                np.zeros((n, 1), dtype=hip.CONTOUR_OBJECT_DTYPE),
                np.zeros(0, dtype=hip.CONTOUR_DTYPE), np.zeros((0, 2), dtype=np.int32))
    mx, nc, npt = C.c_int32(0), C.c_int64(0), C.c_int64(0)
    # a first attempt sized by guess; the call reports what a larger result needs
    per, cap_c, cap_p = 4096, 2 * 4096 * n, max(4096, a.size // 8)
    while True:
        rows = np.empty((n, per), dtype=hip.OBJECT_ROW_DTYPE)
        objects = np.empty((n, per), dtype=hip.CONTOUR_OBJECT_DTYPE)
        contours = np.empty(cap_c, dtype=hip.CONTOUR_DTYPE)
        points = np.empty((cap_p, 2), dtype=np.int32)
        rc = L.tmh_object_contours(hip.ptr(a), n, a.shape[1], a.shape[2], C.byref(mx),
                                   hip.ptr(rows), hip.ptr(objects), rows.size, hip.ptr(contours),
                                   cap_c, hip.ptr(points), cap_p, C.byref(nc), C.byref(npt))
        if rc == hip.TMH_EINVAL and (mx.value + 1 > per or nc.value > cap_c or npt.value > cap_p):
            per, cap_c, cap_p = max(per, mx.value + 1), max(cap_c, nc.value), max(cap_p, npt.value)
            continue
        hip.check(rc)
        k = mx.value + 1
        return (rows.reshape(-1)[:n * k].reshape(n, k), objects.reshape(-1)[:n * k].reshape(n, k),
                contours[:nc.value], points[:npt.value])


def cv2_order(n):
    """List position -> discovery index of the list cv2.findContours returns
    for n borders: reverse discovery order (OpenCV's legacy tracer links a
    later border in front -- DESIGN section 1, rests on reading).  The one
    place that order is decided."""
    return list(range(n - 1, -1, -1))


def cv2_shaped(borders, parents):
    """cv2.findContours' ``(contours, hierarchy)`` from borders (int32 [n, 2]
    arrays) in discovery order and their RETR_CCOMP parents (discovery
    indices, -1 for an outer border): contours a list of [n, 1, 2] arrays,
    hierarchy [1, n, 4] of [next, previous, first child, parent] positions."""
    n = len(borders)
    order = cv2_order(n)
    pos = dict((d, p) for p, d in enumerate(order))
    contours = [np.array(borders[d], dtype=np.int32).reshape(-1, 1, 2) for d in order]
    hierarchy = np.full((1, n, 4), -1, dtype=np.int32)
    last = dict()  # parent position -> the last position seen with that parent
    for p, d in enumerate(order):
        parent = pos[parents[d]] if parents[d] >= 0 else -1
        hierarchy[0, p, 3] = parent
        if parent in last:
            hierarchy[0, p, 1] = last[parent]
            hierarchy[0, last[parent], 0] = p
        elif parent >= 0:
            hierarchy[0, parent, 2] = p
        last[parent] = p
    return contours, hierarchy


def select_shell_and_holes(contours, hierarchy):
    """tmlib/image.py:842-869 as written, for one or more contours: of an
    outer border with holes only its first child is kept; among several outer
    borders without holes the longest is the shell."""
    if len(contours) > 1:
        holes = list()
        for i in range(len(contours)):
            child_idx = hierarchy[0][i][2]
            parent_idx = hierarchy[0][i][3]
            if parent_idx >= 0:
                shell = np.squeeze(contours[parent_idx])
            elif child_idx >= 0:
                holes.append(np.squeeze(contours[child_idx]))
            else:
                lengths = [len(c) for c in contours]
                idx = lengths.index(np.max(lengths))
                shell = np.squeeze(contours[idx])
                break
    else:
        shell = np.squeeze(contours[0])
        holes = None
    return shell, holes


class ContourPolygon(object):
    """What extract_polygons yields where the reference builds a
    ``shapely.geometry.Polygon``: the shell and the holes as int32 [n, 2]
    (x, y) rings, unclosed as cv2 gives them.  The reference's ``is_valid`` /
    ``buffer(0)`` repair (image.py:895-916) is not applied."""

    __slots__ = ("shell", "holes")

    def __init__(self, shell, holes=None):
        self.shell = np.ascontiguousarray(shell, dtype=np.int32).reshape(-1, 2)
        self.holes = [np.ascontiguousarray(h, dtype=np.int32).reshape(-1, 2)
                      for h in (holes or [])]

    def to_shapely(self):
        try:
            import shapely.geometry
        except ImportError:
            from .workflow.align.api import NotSupportedError
            raise NotSupportedError("shapely is not installed: no shapely.geometry.Polygon")
        return shapely.geometry.Polygon(self.shell, self.holes)

    def __eq__(self, other):
        return (isinstance(other, ContourPolygon) and np.array_equal(self.shell, other.shell)
                and len(self.holes) == len(other.holes)
                and all(np.array_equal(a, b) for a, b in zip(self.holes, other.holes)))

    def __ne__(self, other):
        return not self == other

    __hash__ = None

    def __repr__(self):
        return "<ContourPolygon(shell=%d points, holes=%d)>" % (len(self.shell), len(self.holes))


def _square(x, y):
    return np.array([[x - 1, x + 1, x + 1, x - 1, x - 1],
                     [y - 1, y - 1, y + 1, y + 1, y - 1]]).T.astype(np.int32)


def polygons_of_plane(rows, objects, contours, points, y_offset, x_offset):
    """image.py:807-917 from one plane's device result (``object_contours``):
    a generator of (label, ContourPolygon) in ascending label order."""
    for label in np.nonzero(objects["n_interior"] > 0)[0]:
        o, r = objects[label], rows[label]
        table = contours[o["first_contour"]:o["first_contour"] + o["n_contours"]]
        holes = None
        if len(table) == 0:
            # the opening left nothing: the mean of the label's pixels on the
            # border-zeroed plane, in plane coordinates (image.py:835-841)
            y = int(np.float64(o["sum_y"]) / np.float64(o["n_interior"]))
            x = int(np.float64(o["sum_x"]) / np.float64(o["n_interior"]))
            shell = _square(x, y)
        else:
            borders = [points[c["point_offset"]:c["point_offset"] + c["n_points"]] for c in table]
            cv_contours, hierarchy = cv2_shaped(borders, table["parent"])
            shell, holes = select_shell_and_holes(cv_contours, hierarchy)
        if shell.ndim < 2 or shell.shape[0] < 3:
            # image.py:871-882; the reference is Python 2: / on these ints floors
            y, x = (int(r["y1"] - r["y0"]) + 2) // 2, (int(r["x1"] - r["x0"]) + 2) // 2
            shell = _square(x, y)
        add_y = y_offset + int(r["y0"]) - 1
        add_x = x_offset + int(r["x0"]) - 1
        shell[:, 0] = shell[:, 0] + add_x
        shell[:, 1] = -1 * (shell[:, 1] + add_y)
        if holes is not None:
            for i in range(len(holes)):
                holes[i][:, 0] = holes[i][:, 0] + add_x
                holes[i][:, 1] = -1 * (holes[i][:, 1] + add_y)
        yield (int(label), ContourPolygon(shell, holes))


class SegmentationImage(Image):
    """A labeled image, one positive int32 identifier per segmented object
    (tmlib/image.py:696-738).  The reference's ``extract_polygons`` method and
    ``create_from_polygons`` class method are the module's functions
    ``extract_polygons(image, y_offset, x_offset)`` and
    ``create_from_polygons(polygons, y_offset, x_offset, dimensions)``: the
    class itself keeps to the attributes tests/test_jterator_cpu.py pins
    (neither of the two)."""

    __slots__ = ()

    def __init__(self, array, metadata=None):
        super(SegmentationImage, self).__init__(array, metadata)
        if not self.is_int32:
            raise TypeError("Image must have 32-bit integer type.")

    @property
    def is_int32(self):
        return self.array.dtype == np.int32

    @property
    def array(self):
        return self._array

    @array.setter
    def array(self, value):
        if not isinstance(value, np.ndarray):
            raise TypeError('Argument "array" must have type numpy.ndarray.')
        if value.ndim != 2:
            raise ValueError('Argument "array" must be two dimensional.')
        if not value.dtype == np.int32:
            raise ValueError('Argument "array" must have numpy.int32 data type.')
        self._array = value

    def object_table(self):
        """One ``hip.OBJECT_ROW_DTYPE`` row per label 0..max of the plane."""
        return object_tables(self.array[None])[0]

    def bboxes(self):
        """mh.labeled.bbox(self.array) (image.py:796): [max_label + 1, 4] rows
        [min_y, max_y + 1, min_x, max_x + 1], zeros for absent labels."""
        t = self.object_table()
        return np.stack([t["y0"], t["y1"], t["x0"], t["x1"]], axis=1).astype(np.intp)


def extract_polygons(image, y_offset, x_offset):
    """SegmentationImage.extract_polygons of the reference (image.py:778-917)
    for a ``SegmentationImage``: a generator of (label, polygon) in ascending
    label order, the polygon a ``ContourPolygon`` (no shapely repair), from
    one device call -- the object table plus the contours of the plane."""
    if not isinstance(image, SegmentationImage):
        raise TypeError('Argument "image" must have type SegmentationImage.')
    rows, objects, contours, points = object_contours(image.array[None])
    return polygons_of_plane(rows[0], objects[0], contours, points, y_offset, x_offset)


def polygon_ring(geometry):
    """The exterior of one geometry of create_from_polygons as int32 [n, 2]
    global (x, y) pairs: the shell of a ``ContourPolygon``, an [n, 2] integer
    array, or ``np.array(geometry.exterior.coords).astype(int)`` as the
    reference takes a shapely polygon's (image.py:769).  Holes are ignored, as
    there.  An empty ring raises ValueError."""
    if isinstance(geometry, ContourPolygon):
        pts = geometry.shell
    elif hasattr(geometry, "exterior"):
        pts = np.array(geometry.exterior.coords).astype(int)
    else:
        pts = np.asarray(geometry)
        if pts.dtype.kind not in "iu":
            raise TypeError("a ring given as an array must have an integer type")
    if pts.size == 0:
        raise ValueError("an empty ring")
    if pts.ndim != 2 or pts.shape[1] != 2:
        raise ValueError("a ring must be an [n, 2] array of (x, y) pairs")
    if pts.dtype != np.int32:
        if pts.min() < -2 ** 31 or pts.max() > 2 ** 31 - 1:
            raise ValueError("a ring's coordinates must fit 32 bits")
        pts = pts.astype(np.int32)
    return np.ascontiguousarray(pts)


def label_planes_from_polygons(plane_polygons, y_offset, x_offset, dimensions):
    """``create_from_polygons`` for many planes in one ``tmh_polygon_fill``
    call: ``plane_polygons[i]`` is the iterable of (label, geometry) of plane i
    (geometries as ``polygon_ring`` takes them); returns int32 [n, height,
    width] with ``dimensions`` = (height, width).  Within a plane a later
    polygon overwrites an earlier one, as the reference's loop does."""
    height, width = (int(v) for v in dimensions)
    if height <= 0 or width <= 0:
        raise ValueError("dimensions must be positive")
    rings, planes, labels = [], [], []
    n_planes = 0
    for i, polygons in enumerate(plane_polygons):
        n_planes = i + 1
        for label, geometry in polygons:
            label = int(label)
            if not -2 ** 31 <= label <= 2 ** 31 - 1:
                raise ValueError("a label must fit int32")
            rings.append(polygon_ring(geometry))
            planes.append(i)
            labels.append(label)
    out = np.zeros((n_planes, height, width), dtype=np.int32)
    if n_planes == 0:
        return out
    L = hip.lib()
    first = np.zeros(len(rings) + 1, dtype=np.int64)
    if rings:
        np.cumsum([len(r) for r in rings], out=first[1:])
        points = np.ascontiguousarray(np.concatenate(rings, axis=0))
    else:
        points = np.zeros((0, 2), dtype=np.int32)
    plane = np.asarray(planes, dtype=np.int32)
    label = np.asarray(labels, dtype=np.int32)
    hip.check(L.tmh_polygon_fill(hip.ptr(points), hip.ptr(first), hip.ptr(plane), hip.ptr(label),
                                 len(rings), n_planes, height, width, int(y_offset), int(x_offset),
                                 hip.ptr(out)))
    return out


def create_from_polygons(polygons, y_offset, x_offset, dimensions, metadata=None):
    """SegmentationImage.create_from_polygons of the reference
    (image.py:740-776): the label image of (label, geometry) pairs in global
    map coordinates, ``y_offset`` / ``x_offset`` subtracted, drawn on the GPU
    by skimage.draw.polygon's rule.  A module function for
    the reason ``extract_polygons`` is one."""
    planes = label_planes_from_polygons([polygons], y_offset, x_offset, dimensions)
    return SegmentationImage(planes[0], metadata)


class IllumstatsImage(Image):
    """float64 statistics plane (tmlib/image.py:1097-1136)."""

    def __init__(self, array, metadata=None):
        if metadata is not None and not isinstance(metadata, IllumstatsImageMetadata):
            raise TypeError('Argument "metadata" must have type '
                            'tmlib.metadata.IllumstatsImageMetadata.')
        super(IllumstatsImage, self).__init__(array, metadata)
        if not self.is_float:
            raise TypeError("Image must have data type float.")

    @property
    def array(self):
        return self._array

    @array.setter
    def array(self, value):
        if not isinstance(value, np.ndarray):
            raise TypeError('Argument "array" must have type numpy.ndarray.')
        if value.ndim != 2:
            raise ValueError('Argument "array" must be two dimensional.')
        if not value.dtype == np.float64:
            raise ValueError('Argument "array" must have numpy.float data type.')
        self._array = value


class IllumstatsContainer(object):
    """mean/std planes + percentile dict of one channel (tmlib/image.py:1139-1213)."""

    def __init__(self, mean, std, percentiles):
        if not isinstance(mean, IllumstatsImage):
            raise TypeError('Argument "mean" must have type tmlib.image.IllumstatsImage.')
        if not isinstance(std, IllumstatsImage):
            raise TypeError('Argument "std" must have type tmlib.image.IllumstatsImage.')
        self.mean = mean
        self.std = std
        self.percentiles = percentiles
        self._corr = None
        self._corr_key = None
        self._corr_arrays = None
        self._corr_locked = []

    def smooth(self, sigma=5):
        """Gaussian-smooth mean and std in place (image.py:1172-1193)."""
        self.mean.array = self.mean.smooth(sigma).array
        self.mean.metadata.is_smoothed = True
        self.std.array = self.std.smooth(sigma).array
        self.std.metadata.is_smoothed = True
        return self

    def get_closest_percentile(self, value):
        """Value of the percentile whose key is closest to ``value``; the first
        key (in dict order) wins ties (image.py:1195-1213)."""
        keys = np.array(list(self.percentiles.keys()))
        idx = np.abs(keys - value).argmin()
        return self.percentiles[keys[idx]]

    def corrector(self, log_transform=True) -> Corrector:
        """Cached device corrector for the current mean/std planes.

        The cache is keyed on the plane objects AND their contents: building
        the corrector marks both arrays read-only (those that were writeable),
        so an in-place write into ``mean.array`` / ``std.array`` raises
        instead of leaving stale device coefficients behind.  Replacing a
        plane (``smooth`` does) or making it writeable again
        (``arr.flags.writeable = True``, then writing) makes the next call
        rebuild the corrector from the current values.  ``release()`` (also
        run when the container is collected) drops the corrector and makes
        the arrays this container locked writeable again.  Neither closes the
        Corrector itself: a caller may hold it past the container (its own
        ``__del__``/``close`` frees the device handle)."""
        m, s = self.mean.array, self.std.array
        key = (id(m), id(s), bool(log_transform))
        if (self._corr is None or self._corr_key != key or m.flags.writeable or
                s.flags.writeable):
            self.release()
            self._corr = Corrector(m, s, log_transform)
            self._corr_key = key
            self._corr_arrays = (m, s)  # keep the ids valid while cached
            self._corr_locked = [a for a in (m, s) if a.flags.writeable]
            for a in self._corr_locked:
                a.flags.writeable = False
        return self._corr

    def release(self):
        """Drop the cache's reference to the device corrector (a caller that
        still holds it keeps a working handle; the last reference frees it);
        the planes it locked are writeable again (the reference's planes are
        plain arrays)."""
        self._corr = None
        self._corr_key = None
        self._corr_arrays = None
        for a in self._corr_locked:
            try:
                a.flags.writeable = True
            except ValueError:  # a view of a read-only base: leave it
                pass
        self._corr_locked = []

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass
