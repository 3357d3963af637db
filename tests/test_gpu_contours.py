"""GPU: object outlines against the plain-loop literal.

The kernels' per-object records, contour table and points equal
tests/contours_literal.py's exactly on the planes of tests/contour_cases.py
(the host core ran their masks in tests/test_contours_cpu.py), through the
host form, the device form, and the image / handles layer.
"""
import ctypes as C

import numpy as np
import pytest

import contour_cases as cc
import contours_literal as cl

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    from tmlibrary_amd import hip
    return hip.lib()


@pytest.fixture(scope="module")
def torch_():
    import torch
    return torch


def check_layout():
    from tmlibrary_amd import hip
    assert cl.CONTOUR_DTYPE == hip.CONTOUR_DTYPE and cl.OBJECT_DTYPE == hip.CONTOUR_OBJECT_DTYPE


def assert_equal_literal(got, want):
    """(objects, contours, points) of the device against the literal's."""
    objects, contours, points = got
    w_objects, w_contours, w_points = want
    assert objects.shape == w_objects.shape
    for name in cl.OBJECT_DTYPE.names:
        assert np.array_equal(objects[name], w_objects[name]), name
    assert contours.shape == w_contours.shape
    for name in cl.CONTOUR_DTYPE.names:
        assert np.array_equal(contours[name], w_contours[name]), name
    assert points.dtype == np.int32 and points.tobytes() == w_points.tobytes()


def run(planes):
    from tmlibrary_amd.image import object_contours
    rows, objects, contours, points = object_contours(planes)
    return rows, (objects, contours, points)


def by_label(result, label, plane=0):
    objects, contours, points = result
    o = objects[plane][label]
    table = contours[o["first_contour"]:o["first_contour"] + o["n_contours"]]
    return o, table


@pytest.mark.parametrize("name", [n for n, _ in cc.SMALL_PLANES])
def test_small_planes_equal_literal(L, name):
    check_layout()
    planes, want = cc.literal(name)
    assert planes.shape[1] <= 40 and planes.shape[2] <= 150
    rows, got = run(planes)
    assert_equal_literal(got, want)


def test_small_planes_take_the_paths_they_name(L):
    """The literal's own results say that the cases reach what they are for."""
    _, widths = cc.literal("widths")
    planes = cc.literal("widths")[0]
    import objects_literal as ol
    r = ol.object_rows(planes[0])
    assert [int(r[k]["x1"] - r[k]["x0"]) for k in (1, 2, 3, 4)] == [63, 64, 65, 130]
    assert r[5]["x0"] == 62
    _, border = cc.literal("border")
    for label in (2, 4, 7):  # wholly on a border line: nothing
        o, table = by_label(border, label)
        assert o["n_interior"] == 0 and o["n_contours"] == 0
    assert by_label(border, 1)[0]["n_contours"] >= 1 and by_label(border, 3)[0]["n_contours"] >= 1
    _, small = cc.literal("small")
    o, table = by_label(small, 1)  # one pixel: no opening, one point (second fallback)
    assert (o["n_interior"], o["opened"], o["n_contours"], o["n_points"]) == (1, 0, 1, 1)
    for label in (2, 3, 4, 6):     # the opening erases them (first fallback)
        o, table = by_label(small, label)
        assert o["opened"] == 1 and o["n_contours"] == 0 and o["n_interior"] >= 2
    _, rings = cc.literal("rings")
    assert by_label(rings, 1)[1]["is_hole"].tolist() == [0, 1]
    assert by_label(rings, 2)[1]["is_hole"].tolist() == [0, 1, 1, 1]
    assert by_label(rings, 2)[1]["parent"].tolist() == [-1, 0, 0, 0]
    assert by_label(rings, 3)[1]["is_hole"].tolist() == [0, 0]  # the bridge is gone
    assert by_label(rings, 4)[1]["is_hole"].tolist() == [0, 1]
    assert by_label(rings, 5)[1]["is_hole"].tolist() == [0]
    objects = cc.literal("maxlabel")[1][0]
    assert objects.shape == (1, 100001) and int((objects["n_contours"] > 0).sum()) == 3


@pytest.mark.parametrize("which", ["CONTOUR_LDS_PIXELS", "CONTOUR_LDS_SMALL_PIXELS",
                                   "CONTOUR_LDS_TINY_PIXELS"])
def test_each_side_of_the_lds_switch(L, which):
    """One object at the constant and one a column above it: LDS against
    memory, and each LDS form against the next larger one."""
    from tmlibrary_amd import hip
    import objects_literal as ol
    limit = getattr(hip, which)
    planes, want = cc.literal("switch", limit)
    r = ol.object_rows(planes[0])
    box = [int(r[k]["y1"] - r[k]["y0"] + 2) * int(r[k]["x1"] - r[k]["x0"] + 2) for k in (1, 2)]
    side = int(round(limit ** 0.5))
    assert box[0] == limit < box[1] == limit + side
    rows, got = run(planes)
    assert_equal_literal(got, want)
    assert want[0]["n_contours"][0, 1] > 1 and want[0]["n_contours"][0, 2] > 1


def test_single_label_plane(L):
    planes, want = cc.literal("single")
    assert planes.shape == (1, 300, 700)
    rows, got = run(planes)
    assert_equal_literal(got, want)
    assert want[0]["n_contours"][0, 1] > 100  # the enclosed zeros are holes


def test_voronoi_five_planes_one_call(L):
    planes, want = cc.literal("voronoi")
    assert planes.shape == (5, 240, 320)
    rows, got = run(planes)
    assert_equal_literal(got, want)
    # the same as five calls of one plane
    n_c = n_p = 0
    for p in range(5):
        _, (objects, contours, points) = run(planes[p:p + 1])
        k = objects.shape[1]
        for name in ("n_contours", "opened", "n_points", "n_interior", "sum_y", "sum_x"):
            assert np.array_equal(objects[name][0], got[0][name][p, :k]), name
        assert not got[0]["n_contours"][p, k:].any()
        assert np.array_equal(objects["first_contour"][0] + n_c, got[0]["first_contour"][p, :k])
        assert np.array_equal(objects["first_point"][0] + n_p, got[0]["first_point"][p, :k])
        part = got[1][n_c:n_c + len(contours)]
        for name in ("label", "is_hole", "parent", "n_points"):
            assert np.array_equal(contours[name], part[name]), name
        assert np.array_equal(contours["point_offset"] + n_p, part["point_offset"])
        assert np.array_equal(points, got[2][n_p:n_p + len(points)])
        n_c += len(contours)
        n_p += len(points)
    assert n_c == len(got[1]) and n_p == len(got[2])


def test_two_calls_identical_bytes(L):
    planes, _ = cc.literal("voronoi")
    _, a = run(planes[:2])
    _, b = run(planes[:2])
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()


def device_call(L, torch_, planes, max_label, contour_cap, point_cap, fill=0x5A, guard=64):
    """tmh_object_table_device then tmh_object_contours_device on filled
    buffers with guard regions: (rc, n_contours, n_points, objects, contours,
    points as uint8 tensors with their guards)."""
    n, H, W = planes.shape
    n_rows = n * (max_label + 1)
    d_planes = torch_.from_numpy(np.array(planes)).cuda()
    buf = lambda nbytes: torch_.full((guard + nbytes + guard,), fill, dtype=torch_.uint8,  # noqa: E731
                                     device="cuda")
    d_rows, d_obj = buf(n_rows * 48), buf(n_rows * 64)
    d_con, d_pts = buf(contour_cap * 32), buf(point_cap * 8)
    torch_.cuda.synchronize()
    at = lambda t: C.c_void_p(t.data_ptr() + guard)  # noqa: E731
    rc = L.tmh_object_table_device(C.c_void_p(d_planes.data_ptr()), n, H, W, max_label,
                                   at(d_rows), None)
    if rc != 0:
        return rc, 0, 0, d_obj, d_con, d_pts
    nc, npt = C.c_int64(-1), C.c_int64(-1)
    rc = L.tmh_object_contours_device(C.c_void_p(d_planes.data_ptr()), n, H, W, max_label,
                                      at(d_rows), at(d_obj), at(d_con), contour_cap, at(d_pts),
                                      point_cap, C.byref(nc), C.byref(npt), None)
    assert L.tmh_synchronize(None) == 0
    return rc, nc.value, npt.value, d_obj, d_con, d_pts


def test_device_form_equals_literal(L, torch_):
    from tmlibrary_amd import hip
    planes, want = cc.literal("rings")
    n_c, n_p = len(want[1]), len(want[2])
    rc, nc, npt, d_obj, d_con, d_pts = device_call(L, torch_, planes, 6, n_c, n_p)
    assert rc == 0 and (nc, npt) == (n_c, n_p)
    g = 64
    objects = np.frombuffer(d_obj.cpu().numpy()[g:-g].tobytes(), hip.CONTOUR_OBJECT_DTYPE)
    contours = np.frombuffer(d_con.cpu().numpy()[g:-g].tobytes(), hip.CONTOUR_DTYPE)
    points = np.frombuffer(d_pts.cpu().numpy()[g:-g].tobytes(), np.int32).reshape(-1, 2)
    assert_equal_literal((objects.reshape(1, 7), contours, points), want)
    for t in (d_obj, d_con, d_pts):  # no byte outside the exact capacities
        assert bool((t[:g] == 0x5A).all()) and bool((t[-g:] == 0x5A).all())
    # measuring only: the same totals, the objects filled
    d_planes = torch_.from_numpy(np.array(planes)).cuda()
    d_rows = torch_.zeros(7 * 48, dtype=torch_.uint8, device="cuda")
    d_o2 = torch_.zeros(7 * 64, dtype=torch_.uint8, device="cuda")
    torch_.cuda.synchronize()
    assert L.tmh_object_table_device(C.c_void_p(d_planes.data_ptr()), 1, 40, 90, 6,
                                     C.c_void_p(d_rows.data_ptr()), None) == 0
    a, b = C.c_int64(-1), C.c_int64(-1)
    assert L.tmh_object_contours_device(C.c_void_p(d_planes.data_ptr()), 1, 40, 90, 6,
                                        C.c_void_p(d_rows.data_ptr()),
                                        C.c_void_p(d_o2.data_ptr()), None, 0, None, 0,
                                        C.byref(a), C.byref(b), None) == 0
    assert (a.value, b.value) == (n_c, n_p)
    assert d_o2.cpu().numpy().tobytes() == objects.tobytes()


@pytest.mark.parametrize("short", ["contours", "points"])
def test_too_small_capacity_writes_nothing(L, torch_, short):
    from tmlibrary_amd import hip
    planes, want = cc.literal("rings")
    n_c, n_p = len(want[1]), len(want[2])
    caps = (n_c - 1, n_p) if short == "contours" else (n_c, n_p - 1)
    rc, nc, npt, d_obj, d_con, d_pts = device_call(L, torch_, planes, 6, *caps)
    assert rc == hip.TMH_EINVAL and "capacity" in L.tmh_last_error().decode()
    assert (nc, npt) == (n_c, n_p)  # the needed counts are reported
    assert bool((d_con == 0x5A).all()) and bool((d_pts == 0x5A).all())
    # the host form: every capacity is checked before anything is written
    a = np.ascontiguousarray(planes)
    rows = np.full(7, 0x5A5A5A5A, np.int32).repeat(12).view(hip.OBJECT_ROW_DTYPE)
    objects = np.full(7 * 16, 0x5A5A5A5A, np.int32).view(hip.CONTOUR_OBJECT_DTYPE)
    contours = np.full(max(caps[0], 1) * 8, 0x5A5A5A5A, np.int32).view(hip.CONTOUR_DTYPE)
    points = np.full((caps[1], 2), 0x5A5A5A5A, np.int32)
    mx, c1, c2 = C.c_int32(-1), C.c_int64(-1), C.c_int64(-1)
    rc = L.tmh_object_contours(hip.ptr(a), 1, 40, 90, C.byref(mx), hip.ptr(rows), hip.ptr(objects),
                               7, hip.ptr(contours), caps[0], hip.ptr(points), caps[1],
                               C.byref(c1), C.byref(c2))
    assert rc == hip.TMH_EINVAL and (mx.value, c1.value, c2.value) == (6, n_c, n_p)
    for buf in (rows, objects, contours, points):
        assert bool((buf.view(np.int32) == 0x5A5A5A5A).all())
    rc = L.tmh_object_contours(hip.ptr(a), 1, 40, 90, C.byref(mx), hip.ptr(rows), hip.ptr(objects),
                               6, hip.ptr(contours), n_c, hip.ptr(points), n_p, C.byref(c1),
                               C.byref(c2))
    assert rc == hip.TMH_EINVAL and "row capacity" in L.tmh_last_error().decode()
    assert bool((rows.view(np.int32) == 0x5A5A5A5A).all())


@pytest.mark.parametrize("bad,message", [(-1, "negative label"), (8, "above max_label")])
def test_labels_out_of_range_are_rejected(L, torch_, bad, message):
    from tmlibrary_amd import hip
    from tmlibrary_amd.image import object_contours
    plane = (np.arange(40 * 50, dtype=np.int32) % 8).reshape(1, 40, 50)
    plane[0, 17, 23] = bad
    # the device form starts from tmh_object_table_device's rows, which is
    # where the range is checked: nothing reaches the contour buffers
    rc, _, _, d_obj, d_con, d_pts = device_call(L, torch_, plane, 7, 64, 4096)
    assert rc == hip.TMH_EINVAL and message in L.tmh_last_error().decode()
    for t in (d_obj, d_con, d_pts):
        assert bool((t == 0x5A).all())
    if bad < 0:
        with pytest.raises(ValueError, match="negative label"):
            object_contours(plane)


def polygon_tuple(label, polygon):
    return (label, polygon.shell.tobytes(), [h.tobytes() for h in polygon.holes])


@pytest.mark.parametrize("offsets", [(-17, 9), (23, -4)])
def test_polygons_equal_literal(L, offsets):
    from tmlibrary_amd.image import ContourPolygon, SegmentationImage, extract_polygons
    from tmlibrary_amd.workflow.jterator.handles import SegmentedObjects
    value = cc.polygon_value()
    assert value.shape[2:] == (3, 2)
    obj = SegmentedObjects("cells", "cells")
    obj.value = value
    got = list(obj.iter_polygons(*offsets))
    want = cl.iter_polygons(value, *offsets)
    assert len(got) == len(want) > 20
    assert [g[:3] for g in got] == [w[:3] for w in want]
    kinds = set()
    for (t, z, label, polygon), (_, _, _, shell, holes) in zip(got, want):
        assert isinstance(polygon, ContourPolygon)
        assert polygon == ContourPolygon(shell, holes), (t, z, label)
        assert polygon.shell.dtype == np.int32 and type(label) is int
        kinds.add((len(polygon.shell) == 5, len(polygon.holes)))
    assert (True, 0) in kinds and (False, 1) in kinds  # fallback squares and holes both occur
    plane = np.ascontiguousarray(value[:, :, 1, 1])
    one = list(extract_polygons(SegmentationImage(plane), *offsets))
    with pytest.raises(TypeError, match="SegmentationImage"):
        extract_polygons(plane, *offsets)
    assert [polygon_tuple(*p) for p in one] == \
        [polygon_tuple(l, ContourPolygon(s, h)) for l, s, h in cl.extract_polygons(plane, *offsets)]
    assert [polygon_tuple(*g[2:]) for g in got if g[:2] == (1, 1)] == [polygon_tuple(*p) for p in one]
