"""Label image handles of jterator, with the per-object numbers from the GPU.

Mirrors tmlib/workflow/jterator/handles.py: ``LabelImage`` (:334-365) and the
subset of ``SegmentedObjects`` (:399-575) that is computed from the label
planes themselves -- ``labels``, ``iter_points``, ``iter_polygons``,
``is_border`` -- and of the way back, ``add_polygons`` (:481-515), plus
``iter_planes`` (:220-235) and the ``save`` / ``represent_as_polygons`` type
checks.  All planes of a value go through one ``tmh_object_table`` call
(``iter_polygons``: one ``tmh_object_contours`` call, ``add_polygons``: one
``tmh_polygon_fill`` call); the host only does the reference's last arithmetic
on the integer sums and its choice of shell and holes.

``Measurement`` (:840-924) and ``SegmentedObjects.measurements`` /
``add_measurement`` (:577-658) carry per-object feature frames, restated for
pandas 2.3 / numpy 2.2 (``np.nan``; the caller's frame is never mutated);
``workflow/jterator/measure.py`` fills them from the GPU.  pandas is imported
where it is used, so importing the package does not need it.

Not built: the decoding of WKB elements (geometries arrive as rings:
``image.polygon_ring``).
``iter_points`` yields a plain ``(x, y)`` tuple where the reference builds a
``shapely.geometry.Point``, ``iter_polygons`` an ``image.ContourPolygon``.
"""
from __future__ import annotations

import collections
import logging
import re

import numpy as np

from tmlibrary_amd.image import (label_planes_from_polygons, object_contours, object_tables,
                                 polygons_of_plane)

logger = logging.getLogger(__name__)


class LabelImage(object):
    """handles.py:198-235, 334-365: a piped label image, background zero."""

    def __init__(self, name, key, help=""):
        self.name = name
        self.help = help
        self.key = str(key)

    @property
    def type(self):
        return self.__class__.__name__

    @property
    def value(self):
        return self._value

    @value.setter
    def value(self, value):
        if not isinstance(value, np.ndarray):
            raise TypeError('Returned value for "%s" must have type numpy.ndarray.' % self.name)
        if not value.dtype == np.int32:
            raise TypeError('Returned value for "%s" must have data type int32.' % self.name)
        self._value = value
        self._tables = None

    def iter_planes(self):
        """((t, z), plane) for every 2-D plane, t outer, z inner (handles.py:220-235)."""
        array = self.value
        if array.ndim == 2:
            array = array[..., np.newaxis, np.newaxis]
        elif array.ndim == 3:
            array = array[..., np.newaxis]
        for t in range(array.shape[-1]):
            for z in range(array[..., t].shape[-1]):
                yield ((t, z), array[:, :, z, t])

    def __str__(self):
        return "<LabelImage(name=%r, key=%r)>" % (self.name, self.key)


class SegmentedObjects(LabelImage):
    """handles.py:399-575: segmented objects encoded as labels."""

    def __init__(self, name, key, help=""):
        super(SegmentedObjects, self).__init__(name, key, help)
        self._features = collections.defaultdict(list)
        self.save = False
        self.represent_as_polygons = True

    def object_tables(self):
        """{(t, z): rows} -- the GPU's object table of every plane (one call
        for all planes of the value, kept until the value is set again)."""
        if self._tables is None:
            keys, planes = [], []
            for key, plane in self.iter_planes():
                keys.append(key)
                planes.append(plane)
            rows = object_tables(np.stack(planes, axis=0))
            self._tables = collections.OrderedDict(zip(keys, rows))
        return self._tables

    @property
    def labels(self):
        """np.unique(value[value > 0]) (handles.py:424): the labels with at
        least one pixel in any plane."""
        n = None
        for rows in self.object_tables().values():
            n = rows["n"].copy() if n is None else n + rows["n"]
        present = np.nonzero(n > 0)[0]
        return [int(label) for label in present if label > 0]

    def iter_points(self, y_offset, x_offset):
        """handles.py:444-455: per plane mh.center_of_mass(plane, labels=plane)
        -- the plane's own values are the weights, so label L has
        cy = float(L * sum_y) / float(L * n) -- then + offsets, y negated,
        int().  A label of ``labels`` absent from a plane meets NaN there and
        int() raises ValueError, as in the reference."""
        labels = self.labels
        for (t, z), rows in self.object_tables().items():
            for label in labels:
                n, sy, sx = (int(rows[label][k]) for k in ("n", "sum_y", "sum_x"))
                if n == 0:
                    raise ValueError("cannot convert float NaN to integer")
                cy = float(label * sy) / float(label * n)
                cx = float(label * sx) / float(label * n)
                cx += x_offset
                cy += y_offset
                cy *= -1
                yield (t, z, label, (int(cx), int(cy)))

    def iter_polygons(self, y_offset, x_offset):
        """handles.py:457-479: (t, z, label, polygon) per plane in iter_planes
        order, the labels of a plane ascending; all planes of the value go to
        the device in one call."""
        keys, planes = [], []
        for key, plane in self.iter_planes():
            keys.append(key)
            planes.append(plane)
        rows, objects, contours, points = object_contours(np.stack(planes, axis=0))
        for i, (t, z) in enumerate(keys):
            for label, polygon in polygons_of_plane(rows[i], objects[i], contours, points,
                                                    y_offset, x_offset):
                yield (t, z, label, polygon)

    def add_polygons(self, polygons, y_offset, x_offset, dimensions):
        """handles.py:481-515: the label image of ``polygons[t][z]``, each an
        iterable of (label, geometry) in global map coordinates (geometries as
        ``image.polygon_ring`` takes them), drawn for all planes in one device
        call and stacked as the reference stacks them: sets and returns
        ``value``, int32 (height, width, n_zplanes, n_tpoints)."""
        polygons = [list(zpolys) for zpolys in polygons]
        if not polygons or not polygons[0]:
            raise ValueError("need at least one array to stack")
        n_t, n_z = len(polygons), len(polygons[0])
        if any(len(zpolys) != n_z for zpolys in polygons):
            raise ValueError("all input arrays must have the same shape")
        planes = label_planes_from_polygons([p for zpolys in polygons for p in zpolys],
                                            y_offset, x_offset, dimensions)
        stack = planes.reshape((n_t, n_z) + planes.shape[1:])
        self.value = np.ascontiguousarray(stack.transpose(2, 3, 1, 0))
        return self.value

    @property
    def is_border(self):
        """handles.py:518-551: {(t, z, label): touches the plane's first or
        last row or column} for every non-zero label of the plane."""
        mapping = dict()
        for (t, z), rows in self.object_tables().items():
            for label in np.nonzero(rows["n"] > 0)[0]:
                if label != 0:
                    mapping[(t, z, int(label))] = bool(rows["border"][label])
        return mapping

    @property
    def save(self):
        return self._save

    @save.setter
    def save(self, value):
        if not isinstance(value, bool):
            raise TypeError('Attribute "save" must have type bool.')
        self._save = value

    @property
    def represent_as_polygons(self):
        return self._represent_as_polygons

    @represent_as_polygons.setter
    def represent_as_polygons(self, value):
        if not isinstance(value, bool):
            raise TypeError('Attribute "represent_as_polygons" must have type bool.')
        self._represent_as_polygons = value

    @property
    def measurements(self):
        """handles.py:577-588: one DataFrame per time point, the frames added
        for it side by side."""
        import pandas as pd
        if self._features:
            return [pd.concat(self._features[t], axis=1) for t in sorted(self._features.keys())]
        return [pd.DataFrame()]

    @measurements.setter
    def measurements(self, value):
        import pandas as pd
        if not isinstance(value, list):
            raise TypeError('Argument "measurements" must have type list.')
        features = collections.defaultdict(list)
        for i, v in enumerate(value):
            if not isinstance(v, pd.DataFrame):
                raise TypeError('Items of argument "measurements" must have type '
                                'pandas.DataFrame.')
            features[i] = [v]
        self._features = features

    def add_measurement(self, measurement):
        """handles.py:605-658: per time point the frame is brought to
        ``labels`` -- missing labels padded with NaN rows, of duplicated labels
        the first kept, unknown labels removed -- and must then match them."""
        if not isinstance(measurement, Measurement):
            raise TypeError('Argument "measurement" must have type '
                            'tmlib.workflow.jterator.handles.Measurement.')
        labels = self.labels
        for t, val in enumerate(measurement.value):
            if len(val.index) < len(labels):
                logger.warning('missing values for object type "%s" at time point %d',
                               self.key, t)
                val = val.copy()
                for label in labels:
                    if label not in val.index:
                        logger.warning("add NaN values for missing object #%d", label)
                        val.loc[label, :] = np.nan
                val = val.sort_index()
            elif len(val.index) > len(labels):
                if len(np.unique(val.index)) < len(val.index):
                    logger.warning('duplicate values for "%s" at time point %d',
                                   measurement.name, t)
                    logger.info("remove duplicates and keep first")
                    val = val[~val.index.duplicated(keep="first")]
                else:
                    logger.warning('too many values for object type "%s" at time point %d',
                                   self.key, t)
                    unknown = [i for i in val.index if i not in labels]
                    for i in unknown:
                        logger.warning("remove values for object #%d", i)
                    val = val.drop(unknown)
            if len(val.index) != len(labels) or np.any(val.index.values != np.array(labels)):
                raise ValueError('Labels of objects for "%s" at time point %d do not match!'
                                 % (measurement.name, t))
            if len(np.unique(val.columns)) != len(val.columns):
                raise ValueError('Column names of "%s" at time point %d must be unique.'
                                 % (measurement.name, t))
            self._features[t].append(val)

    def __str__(self):
        return "<SegmentedObjects(name=%r, key=%r)>" % (self.name, self.key)


class Measurement(object):
    """handles.py:840-924: a list over time points of DataFrames with one row
    per segmented object and one column per feature."""

    _NAME_PATTERN = re.compile(r"^[A-Za-z0-9_-]+$")

    def __init__(self, name, objects, objects_ref, channel_ref=None, help=""):
        for arg, v, types in (("objects", objects, (str,)), ("objects_ref", objects_ref, (str,)),
                              ("channel_ref", channel_ref, (str, type(None)))):
            if not isinstance(v, types):
                raise TypeError('Argument "%s" must have type %s.'
                                % (arg, " or ".join(t.__name__ for t in types)))
        self.name = name
        self.help = help
        self.objects = objects
        self.objects_ref = objects_ref
        self.channel_ref = channel_ref

    @property
    def type(self):
        return self.__class__.__name__

    @property
    def value(self):
        return self._value

    @value.setter
    def value(self, value):
        import pandas as pd
        if not isinstance(value, list):
            raise TypeError('Value of key "%s" must have type list.' % self.name)
        if not all([isinstance(v, pd.DataFrame) for v in value]):
            raise TypeError('Elements of returned value of "%s" must have type '
                            'pandas.DataFrame.' % self.name)
        for v in value:
            for name in v.columns:
                if not self._NAME_PATTERN.search(name):
                    raise ValueError('Feature name "%s" must only contain '
                                     'alphanumerical characters or underscores or hyphens' % name)
        self._value = value

    def to_dict(self):
        return {"name": self.name, "objects": self.objects, "objects_ref": self.objects_ref,
                "channel_ref": self.channel_ref, "type": self.type, "help": self.help}

    def __str__(self):
        return "<Measurement(name=%r, objects=%r)>" % (self.name, self.objects)
