"""CPU: jterator's host side -- the literal of the per-object rules against
scipy, the handles' checks and plane order, and the window / slot planning of
``load_pipeline_input`` against a numpy restatement of the reference loop."""
from collections import OrderedDict

import numpy as np
import pytest
import scipy.ndimage as ndi

import objects_literal as lit
from tmlibrary_amd import hip
from tmlibrary_amd.image import SegmentationImage
from tmlibrary_amd.models.file import ExperimentStore
from tmlibrary_amd.workflow.jterator import api as japi
from tmlibrary_amd.workflow.jterator.handles import LabelImage, SegmentedObjects


def cells(h, w, n, seed):
    """Voronoi-like cells: every pixel takes the label of the nearest of n seeds
    (labels 1..n), with background 0 where the pixel hash says so."""
    rng = np.random.RandomState(seed)
    sy, sx = rng.randint(0, h, n), rng.randint(0, w, n)
    yy, xx = np.mgrid[0:h, 0:w]
    d = (yy[..., None] - sy) ** 2 + (xx[..., None] - sx) ** 2
    plane = (np.argmin(d, axis=2) + 1).astype(np.int32)
    plane[(yy * 7 + xx * 3) % 11 == 0] = 0
    return plane


# ---- the literal against scipy ---------------------------------------------------

@pytest.mark.parametrize("shape,n,seed,offsets", [((40, 56), 9, 1, (-13, 22)),
                                                  ((37, 57), 14, 2, (5, -3)),
                                                  ((64, 30), 5, 3, (0, 0))])
def test_literal_centroids_match_scipy(shape, n, seed, offsets):
    plane = cells(shape[0], shape[1], n, seed)
    labels = lit.labels(plane)
    assert len(labels) >= 3
    y_off, x_off = offsets
    want = np.asarray(ndi.center_of_mass(plane, plane, labels))  # weights = the plane's values
    got = lit.center_of_mass(plane)[labels]
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=0)
    # the condition on the inputs: no shifted centroid within 1e-9 of an
    # integer, so int()'s truncation cannot differ between the two
    for c in (want, got):
        shifted = np.stack([-(c[:, 0] + y_off), c[:, 1] + x_off], axis=1)
        assert np.all(np.abs(shifted - np.round(shifted)) > 1e-9)
    pts = {label: xy for _, _, label, xy in lit.iter_points(plane, y_off, x_off)}
    for k, label in enumerate(labels):
        assert pts[label] == (int(want[k, 1] + x_off), int(-(want[k, 0] + y_off)))


def test_literal_rows_match_scipy_objects():
    plane = cells(37, 57, 12, 5)
    rows = lit.object_rows(plane)
    slices = ndi.find_objects(plane)
    for label in lit.labels(plane):
        sl = slices[label - 1]
        assert (rows[label]["y0"], rows[label]["y1"]) == (sl[0].start, sl[0].stop)
        assert (rows[label]["x0"], rows[label]["x1"]) == (sl[1].start, sl[1].stop)
        assert rows[label]["n"] == np.count_nonzero(plane == label)
    assert rows[0]["n"] == np.count_nonzero(plane == 0)  # the background has a row too
    border = lit.find_border_objects(plane)
    assert {k for k, v in border.items() if v} == \
        {int(k) for k in np.nonzero(rows["border"])[0] if k != 0}


def test_literal_dtype_is_the_bindings():
    assert lit.ROW_DTYPE == hip.OBJECT_ROW_DTYPE


# ---- type and shape errors -------------------------------------------------------

def test_segmentation_image_errors():
    with pytest.raises(TypeError, match='Argument "array" must have type numpy.ndarray.'):
        SegmentationImage([[1, 2]])
    with pytest.raises(ValueError, match='Argument "array" must be two dimensional.'):
        SegmentationImage(np.zeros((2, 2, 2), np.int32))
    with pytest.raises(ValueError, match='Argument "array" must have numpy.int32 data type.'):
        SegmentationImage(np.zeros((2, 2), np.int64))
    img = SegmentationImage(np.zeros((2, 3), np.int32))
    assert img.dimensions == (2, 3) and img.is_int32
    assert not hasattr(img, "extract_polygons") and not hasattr(img, "create_from_polygons")


def test_segmented_objects_errors():
    obj = SegmentedObjects("cells", "cells")
    assert obj.save is False and obj.represent_as_polygons is True
    with pytest.raises(TypeError, match='Returned value for "cells" must have type numpy.ndarray.'):
        obj.value = [[1]]
    with pytest.raises(TypeError, match='Returned value for "cells" must have data type int32.'):
        obj.value = np.zeros((2, 2), np.uint16)
    with pytest.raises(TypeError, match='Attribute "save" must have type bool.'):
        obj.save = 1
    with pytest.raises(TypeError, match='Attribute "represent_as_polygons" must have type bool.'):
        obj.represent_as_polygons = "yes"
    assert obj.type == "SegmentedObjects" and LabelImage("a", 3).key == "3"


@pytest.mark.parametrize("shape", [(3, 4), (3, 4, 2), (3, 4, 2, 3)])
def test_iter_planes_order(shape):
    value = np.arange(int(np.prod(shape)), dtype=np.int32).reshape(shape)
    obj = LabelImage("x", "x")
    obj.value = value
    got = list(obj.iter_planes())
    want = list(lit.iter_planes(value))
    n_z = shape[2] if len(shape) > 2 else 1
    n_t = shape[3] if len(shape) > 3 else 1
    assert [k for k, _ in got] == [(t, z) for t in range(n_t) for z in range(n_z)]  # t outer
    for (kg, pg), (kw, pw) in zip(got, want):
        assert kg == kw and np.array_equal(pg, pw) and pg.shape == (3, 4)


# ---- window and slot planning ----------------------------------------------------

class FakeStore(ExperimentStore):
    """file_info and alignment results only: nothing on disk is touched."""

    def __init__(self, file_info, shifts, residues):
        super(FakeStore, self).__init__("/nonexistent", file_info)
        self.site_shifts = shifts
        self.site_residues = residues


def shift_and_crop(img, y, x, bottom, top, right, left):
    """tmlib/image.py:380-394 with crop=True."""
    row_start = top - y
    row_end = bottom + y
    row_end = img.shape[0] if row_end == 0 else -row_end
    col_start = left - x
    col_end = right + x
    col_end = img.shape[1] if col_end == 0 else -col_end
    return img[row_start:row_end, col_start:col_end]


def reference_loop(store, site_id, channel_id, planes, shape):
    """jterator/api.py:283-316 for one channel: planes = {file id: array}."""
    n_z, n_t = japi.site_layout(store, site_id)
    res = store.site_residues.get(site_id, dict(bottom=0, top=0, left=0, right=0))
    height = shape[0] - (res["top"] + res["bottom"])
    width = shape[1] - (res["right"] + res["left"])
    image_array = np.zeros((height, width, n_z, n_t), np.uint16)
    for fid in japi.channel_files(store, site_id, channel_id):
        ch, site, cycle, tpoint, zplane = store.file_info[fid]
        y, x = store.site_shifts.get((site, cycle), (0, 0))
        img = shift_and_crop(planes[fid], y, x, res["bottom"], res["top"], res["right"],
                             res["left"])
        image_array[:, :, zplane, tpoint] = img
    return image_array


def make_store():
    # two sites, two cycles (channel 0 in cycle 0, channel 1 in cycle 1), Z = 2, T = 3
    info = OrderedDict()
    fid = 0
    for site in (4, 9):
        for ch, cycle in ((0, 0), (1, 1)):
            for z in range(2):
                for t in range(3):
                    if (ch, z, t) == (1, 1, 2):
                        continue  # one slot of channel 1 has no file: it stays zero
                    info[fid] = (ch, site, cycle, t, z)
                    fid += 1
    shifts = {(4, 0): (0, 0), (4, 1): (3, -2), (9, 0): (0, 0), (9, 1): (-1, 4)}
    residues = {4: dict(bottom=0, top=3, left=0, right=2), 9: dict(bottom=1, top=0, left=4, right=0)}
    return FakeStore(info, shifts, residues)


def test_planning_matches_reference_loop():
    store = make_store()
    shape = (21, 30)
    rng = np.random.RandomState(0)
    planes = {fid: rng.randint(0, 65535, shape).astype(np.uint16) for fid in store.file_info}
    for site in (4, 9):
        n_z, n_t = japi.site_layout(store, site)
        assert (n_z, n_t) == (2, 3)
        for ch in (0, 1):
            files = japi.channel_files(store, site, ch)
            windows, slots, extents = japi.plan_planes(store, files, shape, n_z, n_t)
            height, width = japi.aligned_size(store, site, shape)
            got = np.zeros((height, width, n_z * n_t), np.uint16)
            for w, s, e, fid in zip(windows, slots, extents, files):
                assert tuple(e) == (height, width) == (w["rows"], w["cols"])
                _, _, _, tpoint, zplane = store.file_info[fid]
                assert s == zplane * n_t + tpoint
                got[:, :, s] = planes[fid][w["src_r0"]:w["src_r0"] + height,
                                           w["src_c0"]:w["src_c0"] + width]
            want = reference_loop(store, site, ch, planes, shape)
            assert np.array_equal(got.reshape(height, width, n_z, n_t), want)
            if ch == 1:
                assert not want[:, :, 1, 2].any()


def test_slot_is_the_c_order_offset():
    n_z, n_t = 3, 4
    a = np.zeros((1, 1, n_z, n_t), np.int32)
    for z in range(n_z):
        for t in range(n_t):
            a[0, 0, z, t] = z * n_t + t
    assert np.array_equal(a.reshape(-1), np.arange(n_z * n_t))
    store = FakeStore({0: (0, 1, 0, 3, 2), 1: (0, 1, 0, 0, 0), 2: (0, 1, 0, 1, 1),
                       3: (0, 1, 0, 2, 0)}, {}, {})
    assert japi.site_layout(store, 1) == (3, 4)
    _, slots, _ = japi.plan_planes(store, [0, 1, 2, 3], (8, 8), 3, 4)
    assert slots.tolist() == [2 * 4 + 3, 0, 1 * 4 + 1, 2]


def test_planning_rejects_an_index_beyond_the_layout():
    # two files, both at z-plane 5: one distinct z-plane, index 5 out of bounds
    store = FakeStore({0: (0, 1, 0, 0, 5), 1: (0, 1, 0, 1, 5)}, {}, {})
    assert japi.site_layout(store, 1) == (1, 2)
    with pytest.raises(IndexError, match="index 5 is out of bounds for axis 2 with size 1"):
        japi.plan_planes(store, [0, 1], (8, 8), 1, 2)


def test_pipeline_constructor_checks():
    with pytest.raises(ValueError):
        japi.ImageAnalysisPipeline(1, store=None)
    with pytest.raises(TypeError):
        japi.ImageAnalysisPipeline(1, store=object())
    with pytest.raises(ValueError):
        japi.ImageAnalysisPipeline(1, store=FakeStore({}, {}, {}), decode="fast")
