"""GPU encode of channel image files: HDF5 gzip chunks deflated on the device.

The mirror of device_decode.py.  The reference stores every site with h5py
(tmlib/models/file.py:353-363, tmlib/writers.py:384-387), i.e. libhdf5's
deflate filter runs zlib's deflate on the host, one chunk after another under
the HDF5 lock.  Here libtmhip cuts the device sites into chunk-major raw bytes
(``tmh_gather_chunks_device``), codes every chunk as one zlib stream
(``tmh_deflate_device``) and packs the streams; the compressed bytes cross
PCIe and libtmh5 stores them as they are (``H5Dwrite_chunk``,
``tmh5_write_channel_images_raw_chunks``).  The files read back through
h5py / ``read_channel_image`` and through the GPU reader's strict chunk-index
parse.

No CPU fallback inside: without the library or a GPU the calls raise.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from tmlibrary_amd import hip
from tmlibrary_amd.models.device_decode import grow
from tmlibrary_amd.models.file import h5py_chunk_shape, write_raw_chunks


class DeviceChunkEncoder(object):
    """Deflate [n, H, W] uint8/uint16 sites into a blob of zlib streams and
    the ``tmh_zchunk`` table describing them.

    Device buffers (raw chunks, slots, table, statuses) and the pinned host
    staging of the result are kept across calls in ``slots`` rotating slots and
    grown on demand: the arrays ``deflate`` returns are views of a slot's
    pinned memory, valid until the slot comes round again."""

    def __init__(self, device=None, stream=None, slots=2):
        import torch
        self.torch = torch
        self.device = device if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.stream = stream if stream is not None else torch.cuda.Stream(self.device)
        self.slots = [dict() for _ in range(max(1, slots))]
        self.k = 0

    def deflate(self, sites, chunks=None):
        """``sites``: a device tensor or a numpy array, [n, H, W] (or [H, W])
        uint8 / uint16 (an int16 tensor is taken as the uint16 bits, as the
        site buffers of the statistics pass).  ``chunks`` = (rows, cols), None
        for h5py's own choice (the reference's layout).  Returns (blob, table,
        geom): a uint8 array of the packed streams, a ``hip.ZCHUNK_DTYPE``
        array (image-major, then row-major chunks), geom = (height, width,
        elem_bytes, chunk_rows, chunk_cols)."""
        torch = self.torch
        L = hip.lib()
        slot = self.slots[self.k % len(self.slots)]
        self.k += 1
        with torch.cuda.stream(self.stream):
            if isinstance(sites, np.ndarray):
                if sites.dtype not in (np.uint8, np.uint16):
                    raise ValueError("channel images are uint8/uint16")
                a = np.ascontiguousarray(sites)
                es = a.itemsize
                t = torch.from_numpy(a.view(np.uint8 if es == 1 else np.int16))
                dev = t.to(self.device, non_blocking=False)
            else:
                if sites.dtype not in (torch.uint8, torch.int16, getattr(torch, "uint16", torch.int16)):
                    raise ValueError("channel images are uint8/uint16 (int16 bits)")
                self.stream.wait_stream(torch.cuda.current_stream(self.device))
                dev = sites.to(self.device).contiguous()
                es = dev.element_size()
            if dev.dim() == 2:
                dev = dev[None]
            if dev.dim() != 3:
                raise ValueError("sites must be [n, H, W] or [H, W]")
            n_img, H, W = (int(x) for x in dev.shape)
            if chunks is None:
                chunks = h5py_chunk_shape((H, W), es)
            cr, cc = min(int(chunks[0]), H), min(int(chunks[1]), W)
            if cr <= 0 or cc <= 0:
                raise ValueError("chunk extents must be positive")
            n = n_img * (-(-H // cr)) * (-(-W // cc))
            raw_max = cr * cc * es
            raw_bytes = n * raw_max
            dst_bytes = n * int(L.tmh_deflate_bound(raw_max))
            scr_bytes = int(L.tmh_deflate_scratch_bytes(n, raw_max))
            esz = hip.ZCHUNK_DTYPE.itemsize
            d_tab = grow(slot, "d_tab", n * esz, torch.uint8, self.device)
            d_raw = grow(slot, "d_raw", raw_bytes, torch.uint8, self.device)
            d_dst = grow(slot, "d_dst", dst_bytes, torch.uint8, self.device)
            d_scr = grow(slot, "d_scratch", max(scr_bytes, 16), torch.uint8, self.device)
            d_st = grow(slot, "d_status", n, torch.int32, self.device)
            d_tot = grow(slot, "d_total", 1, torch.int64, self.device)
            sp = C.c_void_p(self.stream.cuda_stream)
            hip.check(L.tmh_gather_chunks_device(C.c_void_p(dev.data_ptr()), n_img, H, W, es, cr, cc,
                                                 C.c_void_p(d_tab.data_ptr()),
                                                 C.c_void_p(d_raw.data_ptr()), sp))
            hip.check(L.tmh_deflate_device(C.c_void_p(d_raw.data_ptr()), raw_bytes,
                                           C.c_void_p(d_tab.data_ptr()), n, raw_max,
                                           C.c_void_p(d_dst.data_ptr()), dst_bytes,
                                           C.c_void_p(d_scr.data_ptr()), d_scr.numel(),
                                           C.c_void_p(d_st.data_ptr()),
                                           C.c_void_p(d_tot.data_ptr()), sp))
            h_tab = grow(slot, "h_tab", n * esz, torch.uint8)
            h_st = grow(slot, "h_status", n, torch.int32)
            h_tot = grow(slot, "h_total", 1, torch.int64)
            h_tab[:n * esz].copy_(d_tab[:n * esz], non_blocking=True)
            h_st[:n].copy_(d_st[:n], non_blocking=True)
            h_tot.copy_(d_tot[:1], non_blocking=True)
            self.stream.synchronize()
            total = int(h_tot[0])
            st = h_st[:n].numpy()
            bad = np.nonzero(st)[0]
            if bad.size:
                raise IOError("chunk %d: %s (%d of %d chunks failed to deflate)"
                              % (int(bad[0]), hip.Z_STATUS.get(int(st[bad[0]]), "error"),
                                 bad.size, n))
            h_blob = grow(slot, "h_blob", total, torch.uint8)
            h_blob[:total].copy_(d_dst[:total], non_blocking=True)
            self.stream.synchronize()
        table = h_tab[:n * esz].numpy().view(hip.ZCHUNK_DTYPE)
        return h_blob[:total].numpy(), table, (H, W, es, cr, cc)


_ENCODERS = {}


def _encoder():
    import torch
    dev = torch.cuda.current_device()
    if dev not in _ENCODERS:
        _ENCODERS[dev] = DeviceChunkEncoder()
    return _ENCODERS[dev]


def deflate_sites(sites, chunks=None):
    """(blob, table, geom) of ``sites`` (``DeviceChunkEncoder.deflate`` of the
    current device's shared encoder: the arrays stay valid for one more call)."""
    return _encoder().deflate(sites, chunks)


def write_channel_images_device(paths, sites, chunks=None, n_threads=None):
    """Write ``sites[i]`` as the channel image file ``paths[i]``, its chunks
    deflated on the GPU (the layout of ``write_channel_image``: ``/array``,
    chunked, gzip level 4 recorded)."""
    paths = list(paths)
    blob, table, geom = deflate_sites(sites, chunks)
    H, W, es, cr, cc = geom
    n_img = len(table) // ((-(-H // cr)) * (-(-W // cc)))
    if n_img != len(paths):
        raise ValueError("%d paths for %d sites" % (len(paths), n_img))
    write_raw_chunks(paths, H, W, 8 * es, cr, cc, blob, table, n_threads)
