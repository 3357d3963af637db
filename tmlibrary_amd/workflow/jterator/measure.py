"""Intensity measurements of segmented objects, taken on the GPU.

The hand-off between jterator's site I/O and the tools: label planes and
intensity planes become one feature row per object.
jterator's module library is not part of the reference tree, so the feature
names are this project's: ``Intensity_{max,mean,min,sum,std}_<channel>``, the
rule behind each in section 27.1.  ``save_measurements`` restates the
feature-value half of ``_save_pipeline_outputs`` (tmlib/workflow/jterator/
api.py:532-565) against the in-memory ``FeatureStore``.

All channels of a call go through one ``tmh_intensity_table_device`` call and
one ``tmh_intensity_features_device`` call; only the feature table comes back
to the host.  Device tensors (torch, uint8 / uint16, or int16 holding uint16
bits as the channel stack does) are read in place where their layout is one
the strides describe -- e.g. slices ``stack[k, :, :, slot]`` of the channel
stack -- and are transposed on the device otherwise.
"""
from __future__ import annotations

import ctypes as C
import logging

import numpy as np

from tmlibrary_amd import hip
from tmlibrary_amd.workflow.jterator.handles import Measurement, SegmentedObjects

logger = logging.getLogger(__name__)

FEATURES = hip.INTENSITY_FEATURES


def feature_names(channel):
    """The five column names of a channel, in the order of the feature table."""
    return ["Intensity_%s_%s" % (f, channel) for f in FEATURES]


def _four(a):
    """an (h, w[, z[, t]]) array or tensor as (h, w, z, t)"""
    if a.ndim not in (2, 3, 4):
        raise ValueError("planes must have shape (h, w), (h, w, z) or (h, w, z, t), got %d "
                         "dimension(s)." % a.ndim)
    while a.ndim < 4:
        a = a[..., None]
    return a


def _is_tensor(a):
    return type(a).__module__.split(".")[0] == "torch"


def _tensor_layout(tensors, elem):
    """(base address, channel, plane, row, pixel stride in elements) when the
    (h, w, z, t) tensors can be read where they are, else None"""
    first = tensors[0]
    sh, sw, sz, st = first.stride()
    n_z, n_t = first.shape[2], first.shape[3]
    if n_z == 1:
        ps = st
    elif n_t == 1 or st == n_z * sz:
        ps = sz
    else:
        return None
    if any(x.stride() != first.stride() for x in tensors):
        return None
    # channels of one allocation only: between two allocations may lie anything,
    # the call's own buffers included
    if any(x.untyped_storage().data_ptr() != first.untyped_storage().data_ptr() for x in tensors):
        return None
    ptrs = [x.data_ptr() for x in tensors]
    cs = 0
    if len(ptrs) > 1:
        step = ptrs[1] - ptrs[0]
        if step < 0 or step % elem or any(b - a != step for a, b in zip(ptrs, ptrs[1:])):
            return None
        cs = step // elem
    return ptrs[0], cs, ps, sh, sw


def _label_planes(objects):
    """-> (int32 [t * z, h, w] planes, (h, w, z, t), object rows or None)"""
    rows = None
    if isinstance(objects, SegmentedObjects):
        value = objects.value
        if objects._tables is not None:
            rows = np.stack(list(objects._tables.values()), axis=0)
    else:
        value = objects
    if not isinstance(value, np.ndarray) or value.dtype != np.int32:
        raise TypeError("objects must be a SegmentedObjects or an int32 numpy.ndarray of labels.")
    four = _four(value)
    h, w, n_z, n_t = four.shape
    if h < 1 or w < 1 or n_z < 1 or n_t < 1:
        raise ValueError("label planes of shape %r hold no pixel." % (value.shape,))
    planes = np.ascontiguousarray(four.transpose(3, 2, 0, 1)).reshape(n_t * n_z, h, w)
    return planes, four.shape, rows


def measure_intensity(objects, images, objects_ref=None):
    """One ``Measurement`` per channel of ``images`` (dict: channel_ref ->
    intensity array of the labels' shape, uint8 or uint16, numpy or device
    tensor) for ``objects``, a ``SegmentedObjects`` or an int32 label array of
    shape (h, w[, z[, t]]).  Each ``value`` is a list over time points of
    DataFrames indexed by the time point's labels (the z-planes of a time
    point are one object) with the columns ``feature_names(channel_ref)``."""
    import pandas as pd
    planes, shape, object_rows = _label_planes(objects)
    h, w, n_z, n_t = shape
    if not isinstance(images, dict) or not images:
        raise TypeError("images must be a non-empty dict of channel name -> intensity array.")
    if len(images) > hip.INTENSITY_MAX_CHANNELS:
        raise ValueError("%d channels: at most %d are measured per call."
                         % (len(images), hip.INTENSITY_MAX_CHANNELS))
    names = list(images)
    for name in names:
        if not isinstance(name, str):
            raise TypeError("channel names must have type str.")
        for column in feature_names(name):
            if not Measurement._NAME_PATTERN.search(column):
                raise ValueError('Feature name "%s" must only contain '
                                 'alphanumerical characters or underscores or hyphens' % column)
    arrays = [images[name] for name in names]
    on_device = [_is_tensor(a) for a in arrays]
    if any(on_device) and not all(on_device):
        raise TypeError("the images of a call are all numpy arrays or all device tensors.")
    if on_device[0]:
        import torch
        kinds = {torch.uint8: 1, torch.uint16: 2, torch.int16: 2}
        if any(not a.is_cuda for a in arrays):
            raise TypeError("image tensors must be on the GPU (or pass numpy arrays).")
    else:
        kinds = {np.dtype(np.uint8): 1, np.dtype(np.uint16): 2}
        arrays = [np.asarray(a) for a in arrays]
    for name, a in zip(names, arrays):
        if a.dtype not in kinds:
            raise TypeError('Image "%s" has data type %s: only uint8 and uint16 images are '
                            'measured.' % (name, a.dtype))
        if kinds[a.dtype] != kinds[arrays[0].dtype]:
            raise TypeError("the images of a call must share one data type.")
        if tuple(_four(a).shape) != tuple(shape):
            raise ValueError('Image "%s" has shape %r, the label image (h, w, z, t) = %r.'
                             % (name, tuple(a.shape), tuple(shape)))
    if object_rows is None:
        if int(planes.min()) < 0:
            raise ValueError("a label plane holds a negative label")
        max_label = int(planes.max())
    else:
        max_label = object_rows.shape[1] - 1
    elem = kinds[arrays[0].dtype]
    n_c, n_planes = len(names), n_t * n_z
    keep = None     # what owns the pixels until the call is complete
    if on_device[0]:
        four = [_four(a) for a in arrays]
        layout = _tensor_layout(four, elem)
        if layout is None:
            keep = torch.stack([x.permute(3, 2, 0, 1) for x in four]).contiguous()
            layout = (keep.data_ptr(), n_planes * h * w, h * w, w, 1)
        else:
            keep = four
        torch.cuda.current_stream().synchronize()   # the tensors' producers are done
    else:
        host = np.ascontiguousarray(np.stack([_four(a).transpose(3, 2, 0, 1) for a in arrays]))
        keep = hip.DeviceBuffer.from_array(host)
        layout = (keep.value, n_planes * h * w, h * w, w, 1)
    L = hip.lib()
    n_rows = n_planes * (max_label + 1) * n_c
    n_feat = n_t * (max_label + 1) * n_c * 5
    buffers = []
    try:
        d_labels = hip.DeviceBuffer.from_array(planes)
        buffers.append(d_labels)
        d_obj = None
        if object_rows is not None:
            d_obj = hip.DeviceBuffer.from_array(object_rows)
            buffers.append(d_obj)
        d_rows = hip.DeviceBuffer(n_rows * hip.INTENSITY_ROW_DTYPE.itemsize)
        buffers.append(d_rows)
        d_feat = hip.DeviceBuffer(n_feat * 8)
        buffers.append(d_feat)
        base, cs, ps, rs, xs = layout
        hip.check(L.tmh_intensity_table_device(d_labels, C.c_void_p(base), elem, n_planes, h, w,
                                               n_c, cs, ps, rs, xs, max_label, d_obj, d_rows,
                                               None))
        hip.check(L.tmh_intensity_features_device(d_rows, n_planes, n_t, max_label, n_c, d_feat,
                                                  None))
        feat = d_feat.get((n_t, max_label + 1, n_c, 5), np.float64)
        hip.check(L.tmh_synchronize(None))
    finally:
        for b in buffers:
            b.free()
        if isinstance(keep, hip.DeviceBuffer):
            keep.free()
        del keep
    key = objects.key if isinstance(objects, SegmentedObjects) else "objects"
    if objects_ref is None:
        objects_ref = key
    measurements = []
    for c, name in enumerate(names):
        frames = []
        for t in range(n_t):
            present = np.flatnonzero(~np.isnan(feat[t, :, c, 1]))
            present = present[present > 0]
            frames.append(pd.DataFrame(feat[t, present, c, :], index=pd.Index(present),
                                       columns=feature_names(name)))
        m = Measurement("Intensity_%s" % name, key, objects_ref, channel_ref=name)
        m.value = frames
        measurements.append(m)
    return measurements


def save_measurements(store, segm_objs, site_id):
    """The feature-value half of ``_save_pipeline_outputs`` (api.py:532-565):
    per time point ``data.round(6)``, one new mapobject per row of the frame
    (its labels, in order) appended to the table of the objects' type in
    ``store``; an empty frame is skipped with a warning.  -> {(site_id, t,
    label): mapobject id}."""
    ids = {}
    for t, data in enumerate(segm_objs.measurements):
        data = data.round(6)  # single!
        if data.empty:
            logger.warning("empty measurement at time point %d", t)
            continue
        new = store.append_mapobjects(segm_objs.key, list(data.columns), data.values)
        for label, i in zip(data.index, new):
            ids[(site_id, t, int(label))] = int(i)
    return ids
