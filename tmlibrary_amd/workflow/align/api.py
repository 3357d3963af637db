"""align step: shifts of every site's cycles against the reference cycle.

Mirrors tmlib/workflow/align/api.py:31-260 ``ImageRegistrator``:
``create_run_batches`` groups the sites into jobs and lists, per job, the
reference cycle's files and every cycle's files of the reference wavelength;
``run_job`` reads them, optionally corrects each cycle's sites with that
cycle's channel statistics, registers every target against its site's
reference and derives the site's four residues from the shifts.

Differences by design (database/cluster orchestration is out of scope): files
are resolved through an ``ExperimentStore``; the cycles' files come in as
``cycle_files`` instead of the ORM queries; the result -- the reference's
``SiteShift`` rows and ``Site.*_residue`` columns -- is returned and kept on
the store (``store.site_shifts`` / ``store.site_residues``).  All pairs of a
block of sites are registered in one batched GPU call.
"""
from __future__ import annotations

import ctypes as C
import logging
from collections import OrderedDict

import numpy as np

from tmlibrary_amd import hip
from tmlibrary_amd.metadata import ChannelImageMetadata
from tmlibrary_amd.models.file import (ExperimentStore, RawChunksUnsupported,
                                       channel_image_shape, read_channel_images)
from tmlibrary_amd.workflow.align import registration as reg

logger = logging.getLogger(__name__)


class NotSupportedError(Exception):
    """tmlib.errors.NotSupportedError"""


class JobDescriptionError(Exception):
    """tmlib.errors.JobDescriptionError"""


class WorkflowError(Exception):
    """tmlib.errors.WorkflowError"""


class AlignBatchArguments(object):
    """tmlib/workflow/align/args.py: the step's batch arguments."""

    def __init__(self, ref_cycle=0, ref_wavelength=None, batch_size=100, illumcorr=False):
        self.ref_cycle = ref_cycle
        self.ref_wavelength = ref_wavelength
        self.batch_size = batch_size
        self.illumcorr = illumcorr


class AlignmentResult(object):
    """What one ``run_job`` computed.

    ``shifts``: {(site_id, cycle_id): (y, x)} -- the reference's SiteShift rows;
    ``residues``: {site_id: {'bottom', 'top', 'left', 'right'}} -- its
    Site.*_residue columns, assigned as align/api.py:252-260 assigns them."""

    def __init__(self):
        self.shifts = OrderedDict()
        self.residues = OrderedDict()

    def update(self, other):
        self.shifts.update(other.shifts)
        self.residues.update(other.residues)


def site_residues(y_shifts, x_shifts):
    """align/api.py:252-260, literally: ``bottom, top, left, right =
    calculate_overlap(...)`` although that returns (top, bottom, right, left).
    So ``top`` holds the largest positive y shift and ``left`` the largest
    positive x shift, which is what keeps ``_shift_and_crop``'s
    ``row_start = top - y`` and ``col_start = left - x`` non-negative."""
    bottom, top, left, right = reg.calculate_overlap(y_shifts, x_shifts)
    return {"bottom": int(bottom), "top": int(top), "left": int(left), "right": int(right)}


def fill_metadata(metadata, result):
    """Set ``y_shift``, ``x_shift`` and the four residues of a
    ``ChannelImageMetadata`` from an ``AlignmentResult`` (or a store that holds
    one), by its site and cycle -- what the reference's ORM supplies to
    ``ChannelImageFile.get`` -- so ``Image.align`` and the illuminati chain's
    ``align_window`` can consume it.  Returns the metadata."""
    if not isinstance(metadata, ChannelImageMetadata):
        raise TypeError('Argument "metadata" must have type ChannelImageMetadata.')
    shifts = getattr(result, "shifts", None)
    if shifts is None:
        shifts, residues = result.site_shifts, result.site_residues
    else:
        residues = result.residues
    y, x = shifts[(metadata.site_id, metadata.cycle_id)]
    res = residues[metadata.site_id]
    metadata.y_shift, metadata.x_shift = int(y), int(x)
    metadata.bottom_residue = int(res["bottom"])
    metadata.top_residue = int(res["top"])
    metadata.left_residue = int(res["left"])
    metadata.right_residue = int(res["right"])
    return metadata


class ImageRegistrator(object):
    """Registration of the sites of different cycles (align/api.py:31-260)."""

    def __init__(self, experiment_id, store=None, block=16, decode="auto", decode_threads=None):
        """block: sites registered per batched GPU call (all their cycles).

        decode: "gpu": the sites' gzip chunks are inflated on the GPU and the
        sites corrected and registered where they land; "host": libhdf5 + zlib
        on the cores, then the host-pointer entry points; "auto": the GPU path
        when the files allow it (uint16, deflate-only chunks), else host."""
        self.experiment_id = experiment_id
        if store is None:
            raise ValueError("an ExperimentStore is required (no database in this build)")
        if not isinstance(store, ExperimentStore):
            raise TypeError('Argument "store" must have type ExperimentStore.')
        if decode not in ("auto", "gpu", "host"):
            raise ValueError('decode must be "auto", "gpu" or "host"')
        self.store = store
        self.block = max(1, int(block))
        self.decode = decode
        self.decode_threads = decode_threads
        self._decoder = None
        self.last_path = None  # "gpu" or "host": how the last job's sites were read

    # ---- jobs --------------------------------------------------------------------
    def create_run_batches(self, args, cycle_files=None, site_ids=None):
        """align/api.py:48-144.  ``cycle_files``: an ordered mapping (or list of
        pairs) cycle id -> {site id: [file ids]} of the reference wavelength,
        in cycle-index order (the reference's queries); ``site_ids``: the
        sites, default every site of any cycle, sorted.  Yields
        ``{'id', 'input_ids': {'reference_file_ids', 'target_file_ids'},
        'illumcorr'}`` with ``target_file_ids`` a dict cycle id -> file ids."""
        cycles = list(cycle_files.items()) if hasattr(cycle_files, "items") else list(cycle_files or [])
        if not (len(cycles) > 1):
            raise NotSupportedError("Alignment requires more than one cycle.")
        if args.ref_cycle >= len(cycles):
            raise JobDescriptionError("Cycle index must not exceed total number of cycles.")
        if site_ids is None:
            site_ids = sorted(set(s for _, files in cycles for s in files))
        site_ids = list(site_ids)
        step = max(1, int(args.batch_size))
        job_count = 0
        for at in range(0, len(site_ids), step):
            batch = site_ids[at:at + step]
            job_count += 1
            input_ids = {"reference_file_ids": list(), "target_file_ids": OrderedDict()}
            for index, (cycle_id, files) in enumerate(cycles):
                if not files:
                    raise ValueError('No image files found for cycle %d and wavelength "%s"'
                                     % (cycle_id, args.ref_wavelength))
                input_ids["target_file_ids"].setdefault(cycle_id, [])
                for s in batch:
                    ids = list(files.get(s, ()))
                    if not ids:
                        # an acquisition may have failed at one site in one cycle
                        logger.warning("no files for site %d and cycle %d", s, cycle_id)
                        continue
                    if index == args.ref_cycle:
                        input_ids["reference_file_ids"].extend(ids)
                    input_ids["target_file_ids"][cycle_id].extend(ids)
            yield {"id": job_count, "input_ids": input_ids, "illumcorr": args.illumcorr}

    def delete_previous_job_output(self):
        """align/api.py:146-155: forget stored shifts and residues."""
        self.store.site_shifts = OrderedDict()
        self.store.site_residues = OrderedDict()

    # ---- reading -----------------------------------------------------------------
    def _stats(self, file_id):
        f = self.store.channel_image_file(file_id)
        sf = self.store.illumstats_file(f.channel_id)
        try:
            return sf.get()
        except (IOError, OSError):
            raise WorkflowError("No illumination statistics file found for channel %d"
                                % f.channel_id)

    def _read_device(self, paths, shape, corrector):
        """The files as a device tensor [n, H, W] (int16 storage of the uint16
        pixels), inflated and, with ``corrector``, corrected on the GPU."""
        import torch
        from tmlibrary_amd.models.device_decode import DeviceChunkDecoder
        H, W = shape
        if self._decoder is None:
            self._decoder = DeviceChunkDecoder(n_threads=self.decode_threads)
        dec = self._decoder
        buf = torch.empty((len(paths), H, W), dtype=torch.int16, device=dec.device)
        dec.decode(paths, buf.data_ptr(), expect=(H, W, 2))
        dec.check()
        if corrector is None:
            return buf
        out = torch.empty_like(buf)
        hip.check(hip.lib().tmh_correct_u16_device(
            corrector._h, C.c_void_p(buf.data_ptr()), C.c_void_p(out.data_ptr()), len(paths), -1,
            -1, C.c_void_p(dec.stream.cuda_stream)))
        dec.stream.synchronize()
        return out

    def _read(self, file_ids, shape, corrector, on_device):
        paths = [self.store.channel_image_file(f).location for f in file_ids]
        if on_device:
            return self._read_device(paths, shape, corrector)
        sites = read_channel_images(paths, self.decode_threads)
        if sites.shape[1:] != tuple(shape):
            raise ValueError("operands could not be broadcast together with shapes %s %s"
                             % (sites.shape[1:], tuple(shape)))
        return sites if corrector is None else corrector.apply(sites)

    # ---- run ---------------------------------------------------------------------
    def run_job(self, batch, assume_clean_state=False):
        """align/api.py:157-260: per (site, cycle) the shift of the cycle's image
        against the site's reference image, per site the residues.  Returns an
        ``AlignmentResult`` and merges it into ``store.site_shifts`` /
        ``store.site_residues``."""
        reference_file_ids = list(batch["input_ids"]["reference_file_ids"])
        target_file_ids = batch["input_ids"]["target_file_ids"]
        cycles = list(target_file_ids.items())
        result = AlignmentResult()
        if not reference_file_ids:
            return self._keep(result)
        for cycle_id, tids in cycles:
            if len(tids) != len(reference_file_ids):
                raise ValueError("cycle %s lists %d files for %d reference files"
                                 % (cycle_id, len(tids), len(reference_file_ids)))
        correctors = {}
        try:
            if batch["illumcorr"]:
                logger.info("correct images for illumination artifacts")
                ref_stats = self._stats(reference_file_ids[0])
                correctors[None] = ref_stats.corrector()
                for cycle_id, tids in cycles:
                    correctors[cycle_id] = self._stats(tids[0]).corrector()
            first = self.store.channel_image_file(reference_file_ids[0]).location
            H, W, dt = channel_image_shape(first)
            on_device = self.decode != "host" and np.dtype(dt) == np.uint16
            if self.decode == "gpu" and not on_device:
                raise RawChunksUnsupported("the GPU path takes uint16 sites")
            for at in range(0, len(reference_file_ids), self.block):
                rids = reference_file_ids[at:at + self.block]
                blocks = [(cycle_id, tids[at:at + self.block]) for cycle_id, tids in cycles]
                try:
                    refs, targets = self._read_block(rids, blocks, (H, W), correctors, on_device)
                except RawChunksUnsupported:
                    if self.decode == "gpu" or not on_device:
                        raise
                    logger.info("channel image files not GPU-decodable: reading on the host")
                    on_device = False
                    refs, targets = self._read_block(rids, blocks, (H, W), correctors, False)
                n_sites = len(rids)
                ref_of = np.tile(np.arange(n_sites, dtype=np.int32), len(blocks))
                y, x = reg.calculate_shifts(targets, refs, ref_of)
                y = y.reshape(len(blocks), n_sites)
                x = x.reshape(len(blocks), n_sites)
                for i, rid in enumerate(rids):
                    site_id = self.store.channel_image_file(rid).site_id
                    logger.info("register images at site %d", site_id)
                    for k, (cycle_id, tids) in enumerate(blocks):
                        tf = self.store.channel_image_file(tids[i])
                        result.shifts[(tf.site_id, cycle_id)] = (int(y[k, i]), int(x[k, i]))
                    logger.info("calculate intersection of sites across cycles")
                    result.residues[site_id] = site_residues(y[:, i], x[:, i])
            self.last_path = "gpu" if on_device else "host"
        finally:
            for c in correctors.values():
                c.close()
        return self._keep(result)

    def _read_block(self, rids, blocks, shape, correctors, on_device):
        refs = self._read(rids, shape, correctors.get(None), on_device)
        parts = [self._read(tids, shape, correctors.get(cycle_id), on_device)
                 for cycle_id, tids in blocks]
        if on_device:
            import torch
            return refs, torch.cat(parts, 0)
        return refs, np.concatenate(parts, 0)

    def _keep(self, result):
        for name, part in (("site_shifts", result.shifts), ("site_residues", result.residues)):
            kept = getattr(self.store, name, None)
            if kept is None:
                kept = OrderedDict()
                setattr(self.store, name, kept)
            kept.update(part)
        return result
