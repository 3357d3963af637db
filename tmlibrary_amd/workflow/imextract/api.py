"""imextract: pixel planes -> channel image files (tmlib/workflow/imextract/api.py).

The reference's ``ImageExtractor.run_job`` (:88-157) reads, for every channel
image file of the batch, the planes its ``file_map`` names (``files``,
``series``, ``planes``) out of the microscope's image files, projects them
with ``np.max(np.dstack(planes), axis=2)`` when there are several (:148-153)
and stores the result with ``ChannelImageFile.put`` (:155-157: gzip HDF5
``/array``).  Here the planes come from a caller-supplied *plane source*
``(filename, series, plane) -> ndarray`` -- the microscope-format readers
(BioFormats, cv2; tmlib/readers.py) are out of scope -- and the two steps
that touch every pixel run on the GPU: the projection
(``tmh_zproject_max_device``) and the deflate coding of the files' chunks
(models/device_encode.py), batched over the files of the job.
"""
from __future__ import annotations

import ctypes as C
import logging
import os
from collections import OrderedDict

import numpy as np

from tmlibrary_amd import hip
from tmlibrary_amd.models.file import ExperimentStore, write_channel_images

logger = logging.getLogger(__name__)


def _project_device(stack):
    """[n, z, H, W] uint8/uint16 -> the device tensor [n, H, W] of the maxima."""
    import torch
    n, z, H, W = stack.shape
    es = stack.itemsize
    dev = torch.device("cuda", torch.cuda.current_device())
    tdt = torch.uint8 if es == 1 else torch.int16
    planes = torch.from_numpy(stack.view(np.uint8 if es == 1 else np.int16)).to(dev)
    out = torch.empty((n, H, W), dtype=tdt, device=dev)
    s = torch.cuda.current_stream(dev)
    hip.check(hip.lib().tmh_zproject_max_device(C.c_void_p(planes.data_ptr()), n, z, H, W, es,
                                                C.c_void_p(out.data_ptr()),
                                                C.c_void_p(s.cuda_stream)))
    s.synchronize()
    return out


class ImageExtractor(object):
    """Extraction of pixel planes into channel image files
    (imextract/api.py:37-191) over an ``ExperimentStore``."""

    def __init__(self, experiment_id, store=None, file_maps=None, plane_source=None,
                 encode="auto"):
        """file_maps: an ordered mapping channel image file id -> its
        ``file_map`` ``{'files': [...], 'series': [...], 'planes': [...]}``
        (the reference's ChannelImageFile.file_map).  plane_source: a callable
        ``(filename, series, plane) -> 2-D uint8/uint16 ndarray``.  encode:
        "gpu": projection and deflate on the GPU; "host": numpy and libhdf5's
        filter on the cores, as the reference; "auto": "gpu" when a device is
        present."""
        self.experiment_id = experiment_id
        if store is None:
            raise ValueError("an ExperimentStore is required (no database in this build)")
        if not isinstance(store, ExperimentStore):
            raise TypeError('Argument "store" must have type ExperimentStore.')
        if encode not in ("auto", "gpu", "host"):
            raise ValueError('encode must be "auto", "gpu" or "host"')
        self.store = store
        self.file_maps = OrderedDict(file_maps or {})
        self.plane_source = plane_source
        self.encode = encode
        self.last_path = None  # "gpu" or "host": how the last job's files were written

    @staticmethod
    def _create_batches(li, n):
        n = max(1, int(n))
        return [li[i:i + n] for i in range(0, len(li), n)]

    def create_run_batches(self, args):
        """imextract/api.py:53-71."""
        file_ids = list(self.file_maps)
        for i, ids in enumerate(self._create_batches(file_ids, args.batch_size)):
            yield {"id": i + 1, "channel_image_file_ids": ids}

    def create_collect_batch(self, args):
        """imextract/api.py:73-86."""
        return {"delete": args.delete}

    def _planes(self, fid):
        fmap = self.file_maps[fid]
        planes = []
        for j, filename in enumerate(fmap["files"]):
            plane_ix, series_ix = fmap["planes"][j], fmap["series"][j]
            logger.debug("extract pixel plane #%d of series #%d from file: %s", plane_ix,
                         series_ix, filename)
            planes.append(np.asarray(self.plane_source(filename, series_ix, plane_ix)))
        if not planes:
            raise IndexError("list index out of range")  # the reference's planes[0]
        if len(set(p.shape for p in planes)) > 1:
            np.dstack(planes)  # the reference's error for planes of different shapes
        dt = np.result_type(*planes)  # np.dstack's dtype
        if dt not in (np.uint8, np.uint16) or planes[0].ndim != 2:
            raise ValueError("channel images are 2-D uint8/uint16")
        return [np.ascontiguousarray(p, dtype=dt) for p in planes]

    def run_job(self, batch, assume_clean_state=False, encode=None):
        """imextract/api.py:88-157: the planes of every file of the batch,
        their maximum where a file maps to several, the files written.
        ``encode`` overrides the extractor's for this job."""
        if self.plane_source is None:
            raise ValueError("a plane source is required (no microscope readers in this build)")
        encode = self.encode if encode is None else encode
        if encode not in ("auto", "gpu", "host"):
            raise ValueError('encode must be "auto", "gpu" or "host"')
        if encode == "auto":
            try:
                hip.lib()
                encode = "gpu"
            except hip.HipUnavailableError:
                encode = "host"
        groups = OrderedDict()  # files of one shape, dtype and depth go through the GPU together
        for fid in batch["channel_image_file_ids"]:
            logger.info("extract pixels for channel image file #%d", fid)
            planes = self._planes(fid)
            key = (planes[0].shape, planes[0].dtype.str, len(planes))
            groups.setdefault(key, []).append((fid, planes))
        for (_, _, z), members in groups.items():
            paths = [self.store.channel_image_file(fid).location for fid, _ in members]
            for p in paths:
                os.makedirs(os.path.dirname(p), exist_ok=True)
            stack = np.stack([np.stack(pl) for _, pl in members])  # [n, z, H, W]
            if encode == "gpu":
                if z > 1:
                    logger.info("perform maximumn intensity projection")
                    sites = _project_device(stack)
                else:
                    sites = stack[:, 0]
            else:
                sites = np.max(stack, axis=1) if z > 1 else stack[:, 0]
            logger.info("write pixels to file on disk")
            write_channel_images(paths, sites, encode=encode)
        self.last_path = encode

    def delete_previous_job_output(self):
        """imextract/api.py:159-168: remove the channel image files."""
        for fid in self.file_maps:
            p = self.store.channel_image_file(fid).location
            if os.path.exists(p):
                os.remove(p)

    def collect_job_output(self, batch):
        """imextract/api.py:170-191: the microscope image files are the plane
        source's to delete; nothing is stored here."""
        if batch["delete"]:
            logger.info("delete all microscope image files")
