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

Not built: measurements and the decoding of WKB elements (geometries arrive
as rings: ``image.polygon_ring``).
``iter_points`` yields a plain ``(x, y)`` tuple where the reference builds a
``shapely.geometry.Point``, ``iter_polygons`` an ``image.ContourPolygon``.
"""
from __future__ import annotations

import collections

import numpy as np

from tmlibrary_amd.image import (label_planes_from_polygons, object_contours, object_tables,
                                 polygons_of_plane)


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

    def __str__(self):
        return "<SegmentedObjects(name=%r, key=%r)>" % (self.name, self.key)
