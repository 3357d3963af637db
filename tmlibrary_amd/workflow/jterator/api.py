"""jterator step: a site's pipeline input, loaded on the GPU.

Mirrors tmlib/workflow/jterator/api.py:237-348 (``_load_pipeline_input``): per
site and channel every file (z-plane x time point) is read, corrected with
the channel's statistics when asked, aligned (shifted and cropped) and written
to ``image_array[:, :, f.zplane, f.tpoint]`` of an ``(aligned_height,
aligned_width, n_zplanes, n_tpoints)`` array.  Here all planes of a channel --
of one site or of a batch of sites -- are inflated on the GPU where the files
allow it and go through ONE stack launch (``tmh_correct_stack_u16_device``),
which corrects, crops and interleaves them.

Differences by design: files are resolved through an ``ExperimentStore``
(``file_info``: file id -> (channel_id, site_id, cycle_id, tpoint, zplane);
``site_shifts`` / ``site_residues`` as the align step keeps them;
``channel_names``: optional name -> channel id, default ``int(name)``).  8-bit
channels take the existing host path (``tmh_correct_u8`` + ``tmh_align``).
``objects_input`` (api.py:319-339) reads a site's stored outlines from the
store's optional ``segmentations``: {(name, site_id, tpoint, zplane): [(label,
ring), ...]} -- what ``MapobjectType.get_segmentations_per_site`` returns, the
geometries as rings (``image.polygon_ring``) -- and draws all planes of an
object type in one device call; ``site_offsets``: optional {site_id: (y, x)}
of ``Site.offset``, default (0, 0).  Running the pipeline and saving its
outputs are not built.
"""
from __future__ import annotations

import ctypes as C
import logging

import numpy as np

from tmlibrary_amd import hip
from tmlibrary_amd.image import align_array, align_window, correct_stack
from tmlibrary_amd.metadata import ChannelImageMetadata
from tmlibrary_amd.models.file import (ExperimentStore, RawChunksUnsupported,
                                       channel_image_shape, read_channel_images)
from tmlibrary_amd.workflow.align.api import fill_metadata
from tmlibrary_amd.workflow.jterator.handles import SegmentedObjects

logger = logging.getLogger(__name__)


class PipelineDescriptionError(Exception):
    """tmlib.errors.PipelineDescriptionError"""


def site_layout(store, site_id):
    """(n_zplanes, n_tpoints) of a site: the distinct z-planes and time points
    of ALL its files (jterator/api.py:258-267)."""
    zs, ts = set(), set()
    for info in store.file_info.values():
        if info[1] == site_id:
            ts.add(info[3])
            zs.add(info[4])
    return len(zs), len(ts)


def site_planes(store, site_id):
    """(sorted z-planes, sorted time points) of ALL files of a site."""
    zs, ts = set(), set()
    for info in store.file_info.values():
        if info[1] == site_id:
            ts.add(info[3])
            zs.add(info[4])
    return sorted(zs), sorted(ts)


def aligned_offset(store, site_id):
    """Site.aligned_offset (tmlib/models/site.py:175-182): the site's offset in
    the map plus its top and left residue."""
    y, x = (getattr(store, "site_offsets", None) or {}).get(site_id, (0, 0))
    res = (getattr(store, "site_residues", None) or {}).get(site_id)
    if res is None:
        return int(y), int(x)
    return int(y) + int(res["top"]), int(x) + int(res["left"])


def channel_files(store, site_id, channel_id):
    """File ids of one site and channel, in id order."""
    return sorted(f for f, info in store.file_info.items()
                  if info[1] == site_id and info[0] == channel_id)


def plan_planes(store, file_ids, shape, n_zplanes, n_tpoints):
    """Per file its crop=True alignment window and slot
    ``zplane * n_tpoints + tpoint`` (the C-order offset of
    ``image_array[:, :, zplane, tpoint]``), from the store's alignment
    metadata; sites without stored shifts are not shifted.  Returns (windows,
    slots, (aligned_height, aligned_width) per file)."""
    shifts = getattr(store, "site_shifts", None) or {}
    windows = np.zeros(len(file_ids), dtype=hip.WINDOW_DTYPE)
    slots = np.zeros(len(file_ids), dtype=np.int32)
    extents = []
    for i, fid in enumerate(file_ids):
        f = store.channel_image_file(fid)
        md = ChannelImageMetadata(channel_id=f.channel_id, site_id=f.site_id, tpoint=f.tpoint,
                                  zplane=f.zplane, cycle_id=f.cycle_id)
        if (f.site_id, f.cycle_id) in shifts:
            fill_metadata(md, store)
        for axis, index, size in ((2, f.zplane, n_zplanes), (3, f.tpoint, n_tpoints)):
            if not (-size <= index < size):
                raise IndexError("index %d is out of bounds for axis %d with size %d"
                                 % (index, axis, size))
        w, extent = align_window(shape, md.y_shift, md.x_shift, md.bottom_residue, md.top_residue,
                                 md.right_residue, md.left_residue, crop=True)
        windows[i] = w
        slots[i] = (f.zplane % n_zplanes) * n_tpoints + (f.tpoint % n_tpoints)
        extents.append(extent)
    return windows, slots, extents


def aligned_size(store, site_id, shape):
    """Site.aligned_height / aligned_width (tmlib/models/site.py:162-173)."""
    res = (getattr(store, "site_residues", None) or {}).get(site_id)
    if res is None:
        return int(shape[0]), int(shape[1])
    return (int(shape[0]) - (res["top"] + res["bottom"]),
            int(shape[1]) - (res["right"] + res["left"]))


class ImageAnalysisPipeline(object):
    """The input half of jterator's ``ImageAnalysisPipeline``."""

    def __init__(self, experiment_id, store=None, decode="auto", decode_threads=None):
        """decode: as ``ImageRegistrator``: "gpu" inflates the files' gzip
        chunks on the GPU, "host" reads them with libhdf5, "auto" takes the
        GPU path when the files allow it."""
        self.experiment_id = experiment_id
        if store is None:
            raise ValueError("an ExperimentStore is required (no database in this build)")
        if not isinstance(store, ExperimentStore):
            raise TypeError('Argument "store" must have type ExperimentStore.')
        if decode not in ("auto", "gpu", "host"):
            raise ValueError('decode must be "auto", "gpu" or "host"')
        self.store = store
        self.decode = decode
        self.decode_threads = decode_threads
        self._decoder = None
        self.last_path = None  # "gpu" or "host": how the last call's files were read

    def _channel_id(self, name):
        names = getattr(self.store, "channel_names", None) or {}
        return int(names[name]) if name in names else int(name)

    def _stats(self, name, channel_id):
        try:
            return self.store.illumstats_file(channel_id).get()
        except (IOError, OSError):
            raise PipelineDescriptionError(
                'No illumination statistics file found for channel "%s"' % name)

    def _stack_device(self, paths, shape, corrector, site, slot, windows, n_sites, slots, out):
        """Inflate on the GPU, then the stack launch where the planes land."""
        import torch
        from tmlibrary_amd.models.device_decode import DeviceChunkDecoder
        H, W = shape
        if self._decoder is None:
            self._decoder = DeviceChunkDecoder(n_threads=self.decode_threads)
        dec = self._decoder
        buf = torch.empty((len(paths), H, W), dtype=torch.int16, device=dec.device)
        dec.decode(paths, buf.data_ptr(), expect=(H, W, 2))
        dec.check()
        dev = torch.empty(out.shape, dtype=torch.int16, device=dec.device)
        hip.check(hip.lib().tmh_correct_stack_u16_device(
            None if corrector is None else corrector._h, C.c_void_p(buf.data_ptr()),
            C.c_void_p(dev.data_ptr()), len(paths), H, W, hip.ptr(site), hip.ptr(slot),
            hip.ptr(windows), n_sites, slots, out.shape[1], out.shape[2],
            C.c_void_p(dec.stream.cuda_stream)))
        dec.stream.synchronize()
        out.view(np.int16)[...] = dev.cpu().numpy()

    def _channel_stacks(self, site_ids, layouts, name, correct):
        """[n_sites, height, width, n_zplanes, n_tpoints] of one channel."""
        channel_id = self._channel_id(name)
        files, site_index = [], []
        for k, site_id in enumerate(site_ids):
            ids = channel_files(self.store, site_id, channel_id)
            files.extend(ids)
            site_index.extend([k] * len(ids))
        if not files:
            raise ValueError('No image files found for channel "%s"' % name)
        paths = [self.store.channel_image_file(f).location for f in files]
        H, W, dt = channel_image_shape(paths[0])
        dt = np.dtype(dt)
        n_z, n_t = layouts[0]
        windows, slot, extents = plan_planes(self.store, files, (H, W), n_z, n_t)
        height, width = aligned_size(self.store, site_ids[0], (H, W))
        for k, site_id in enumerate(site_ids):
            if layouts[k] != (n_z, n_t) or aligned_size(self.store, site_id, (H, W)) != (height, width):
                raise ValueError("the sites of a batch must share their aligned size, z-planes "
                                 "and time points")
        for extent in extents:
            if tuple(extent) != (height, width):
                # the reference's image_array[:, :, z, t] = img.array
                raise ValueError("could not broadcast input array from shape (%d,%d) into shape "
                                 "(%d,%d)" % (extent[0], extent[1], height, width))
        stats = None
        if correct:
            logger.info('load illumination statistics for channel "%s"', name)
            stats = self._stats(name, channel_id)
        logger.info('load images for channel "%s"', name)
        site = np.asarray(site_index, dtype=np.int32)
        n_sites, slots = len(site_ids), n_z * n_t
        out = np.zeros((n_sites, height, width, slots), dtype=dt)
        corrector = stats.corrector() if stats is not None else None
        try:
            if dt == np.uint16:
                on_device = self.decode != "host"
                if on_device:
                    try:
                        self._stack_device(paths, (H, W), corrector, site, slot, windows, n_sites,
                                           slots, out)
                    except RawChunksUnsupported:
                        if self.decode == "gpu":
                            raise
                        logger.info("channel image files not GPU-decodable: reading on the host")
                        on_device = False
                if not on_device:
                    planes = read_channel_images(paths, self.decode_threads)
                    out = correct_stack(corrector, planes, site, slot, windows, n_sites, slots,
                                        (height, width))
                self.last_path = "gpu" if on_device else "host"
            else:
                # 8-bit channels: the existing host entry points, plane by plane
                if self.decode == "gpu":
                    raise RawChunksUnsupported("the GPU path takes uint16 sites")
                planes = read_channel_images(paths, self.decode_threads)
                if corrector is not None:
                    planes = corrector.apply(planes)
                for p in range(len(files)):
                    out[site[p], :, :, slot[p]] = align_array(planes[p], windows[p], (height, width))
                self.last_path = "host"
        finally:
            if corrector is not None:
                corrector.close()
        return out.reshape(n_sites, height, width, n_z, n_t)

    def _site_objects(self, site_id, name):
        """api.py:319-339 for one site and object type: the SegmentedObjects
        with its value drawn from the stored outlines."""
        zplanes, tpoints = site_planes(self.store, site_id)
        segmentations = getattr(self.store, "segmentations", None) or {}
        polygons = [[segmentations.get((name, site_id, t, z), []) for z in zplanes]
                    for t in tpoints]
        ids = sorted(f for f, info in self.store.file_info.items() if info[1] == site_id)
        if not ids:
            raise ValueError("No image files found for site %r" % (site_id,))
        H, W, _ = channel_image_shape(self.store.channel_image_file(ids[0]).location)
        y_offset, x_offset = aligned_offset(self.store, site_id)
        segm_obj = SegmentedObjects(name, name)
        segm_obj.add_polygons(polygons, y_offset, x_offset,
                              aligned_size(self.store, site_id, (H, W)))
        return segm_obj

    def load_pipeline_inputs(self, site_ids, channels, objects=()):
        """``load_pipeline_input`` for a batch of sites with one stack launch
        per channel; one store dict per site.  The sites must share their
        aligned size and (n_zplanes, n_tpoints).  ``objects``: names of object
        types whose stored outlines become label images (one device call per
        site and name)."""
        site_ids = list(site_ids)
        logger.info("load pipeline inputs")
        stores = [{"site_id": s, "pipe": dict(), "current_figure": list(), "objects": dict(),
                   "channels": list()} for s in site_ids]
        if not site_ids:
            return stores
        layouts = [site_layout(self.store, s) for s in site_ids]
        for name, correct in channels:
            stacks = self._channel_stacks(site_ids, layouts, name, bool(correct))
            for k, st in enumerate(stores):
                # single dimensions removed, as the reference does (api.py:345-346)
                st["pipe"][name] = np.squeeze(stacks[k])
        for name in objects:
            logger.info('load objects "%s"', name)
            for st in stores:
                segm_obj = self._site_objects(st["site_id"], name)
                st["objects"][segm_obj.name] = segm_obj
                st["pipe"][segm_obj.name] = np.squeeze(segm_obj.value)
        return stores

    def load_pipeline_input(self, site_id, channels, objects=()):
        """jterator/api.py:237-348 for ``channels`` = [(name, correct), ...]
        and ``objects`` = [name, ...]: {'site_id', 'pipe': {name: array},
        'current_figure', 'objects': {name: SegmentedObjects}, 'channels'}."""
        return self.load_pipeline_inputs([site_id], channels, objects)[0]
