"""GPU: label planes from outlines against the plain-loop literal.

The device's planes equal tests/polygons_literal.py's byte for byte on the
cases of that module (the host core ran them in tests/test_polygons_cpu.py),
through the host form, the device form, and the image / handles / api layer.
"""
import ctypes as C
import os

import numpy as np
import pytest

import polygons_literal as pl

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    from tmlibrary_amd import hip
    return hip.lib()


@pytest.fixture(scope="module")
def torch_():
    import torch
    return torch


def run(name):
    from tmlibrary_amd.image import label_planes_from_polygons
    planes, y_offset, x_offset, dims = pl.CASES[name]
    return label_planes_from_polygons(planes, y_offset, x_offset, dims)


def flat(planes):
    """(points, first, plane, label) of plane_polygons, as the C-ABI takes them"""
    rings = [np.asarray(r, np.int32).reshape(-1, 2) for polys in planes for _, r in polys]
    first = np.zeros(len(rings) + 1, np.int64)
    first[1:] = np.cumsum([len(r) for r in rings])
    points = np.ascontiguousarray(np.concatenate(rings)) if rings else np.zeros((0, 2), np.int32)
    plane = np.array([i for i, polys in enumerate(planes) for _ in polys], np.int32)
    label = np.array([l for polys in planes for l, _ in polys], np.int64).astype(np.int32)
    return points, first, plane, label


@pytest.mark.parametrize("name", list(pl.CASES))
def test_cases_equal_literal(L, name):
    got, want = run(name), pl.literal(name)
    assert got.dtype == np.int32 and got.shape == want.shape
    assert got.tobytes() == want.tobytes()


def test_anchors_by_hand(L):
    for k, (_, shape, pixels) in enumerate(pl.ANCHORS):
        assert np.array_equal(run("anchor%d" % k)[0], pl.anchor_plane(shape, pixels)), k


def test_later_polygon_wins_in_both_orders(L):
    ab, ba = run("overlap_ab")[0], run("overlap_ba")[0]
    both = (ab != 0) & (ab != ba)
    assert both.sum() > 50 and (ab[both] == 22).all() and (ba[both] == 11).all()


def test_two_calls_identical_bytes(L):
    for name in ("random300", "stack", "width129_mem"):
        assert run(name).tobytes() == run(name).tobytes()


def test_create_from_polygons_types(L):
    from tmlibrary_amd import image
    from tmlibrary_amd.metadata import SiteImageMetadata
    md = SiteImageMetadata(site_id=3, tpoint=0, zplane=1)
    polygons, y_offset, x_offset, dims = pl.CASES["random300"]
    img = image.create_from_polygons(iter(polygons[0]), y_offset, x_offset, dims)
    assert isinstance(img, image.SegmentationImage) and img.metadata is None
    assert img.array.tobytes() == pl.literal("random300")[0].tobytes()
    wrapped = [(l, image.ContourPolygon(r, [r[:3]])) for l, r in polygons[0]]  # holes are ignored
    img = image.create_from_polygons(wrapped, y_offset, x_offset, dims, metadata=md)
    assert img.metadata is md and img.array.tobytes() == pl.literal("random300")[0].tobytes()
    assert not image.create_from_polygons([], 0, 0, (5, 6)).array.any()


def test_round_trip_of_extracted_outlines(L):
    """extract_polygons -> create_from_polygons on a 128 x 128 plane of blobs
    equals the literal on the same rings; no pixel is gained: every filled
    pixel carries its label in the original plane (the rule leaves out most
    pixels of an outline itself, so pixels are lost)."""
    from tmlibrary_amd import image
    plane = pl.blobs_plane(5, (128, 128), 40)
    n = int(plane.max())
    assert n == 40
    y_offset, x_offset = 3000, -700
    polygons = list(image.extract_polygons(image.SegmentationImage(plane), y_offset, x_offset))
    assert [l for l, _ in polygons] == list(range(1, n + 1))
    got = image.create_from_polygons(polygons, y_offset, x_offset, plane.shape).array
    want = pl.create_from_polygons([(l, p.shell) for l, p in polygons], y_offset, x_offset,
                                   plane.shape)
    assert got.tobytes() == want.tobytes()
    filled = got != 0
    assert ((got[filled] == plane[filled]) | (plane[filled] == 0)).all()
    assert 0 < filled.sum() < (plane != 0).sum()
    assert sorted(np.unique(got[filled])) == list(range(1, n + 1))


def device_call(L, torch_, planes, y_offset, x_offset, dims, n_planes=None, stream=None,
                fill=0x5A, guard=64, edit=None):
    """The device form on guarded buffers: (rc, planes_out int32, guards intact)."""
    points, first, plane, label = flat(planes)
    if edit:
        edit(points, first, plane, label)
    n_planes = len(planes) if n_planes is None else n_planes
    H, W = dims
    dev = [torch_.from_numpy(a.reshape(-1).view(np.uint8).copy()).cuda()
           for a in (points, first, plane, label)]
    nbytes = n_planes * H * W * 4
    out = torch_.full((guard + nbytes + guard,), fill, dtype=torch_.uint8, device="cuda")
    torch_.cuda.synchronize()
    rc = L.tmh_polygon_fill_device(*[C.c_void_p(d.data_ptr()) for d in dev], len(plane), n_planes,
                                   H, W, y_offset, x_offset, C.c_void_p(out.data_ptr() + guard),
                                   None if stream is None else C.c_void_p(stream.cuda_stream))
    torch_.cuda.synchronize()
    raw = out.cpu().numpy()
    intact = (raw[:guard] == fill).all() and (raw[guard + nbytes:] == fill).all()
    return rc, raw[guard:guard + nbytes].view(np.int32).reshape(n_planes, H, W), intact


@pytest.mark.parametrize("name", ["stack", "random300", "width65_mem", "threshold_above"])
def test_device_form_on_a_stream(L, torch_, name):
    planes, y_offset, x_offset, dims = pl.CASES[name]
    stream = torch_.cuda.Stream()
    rc, got, intact = device_call(L, torch_, planes, y_offset, x_offset, dims, stream=stream)
    assert rc == 0, L.tmh_last_error()
    assert intact and got.tobytes() == pl.literal(name).tobytes()
    # the default stream, and an output that is only 4-byte aligned
    rc, again, intact = device_call(L, torch_, planes, y_offset, x_offset, dims, guard=68)
    assert rc == 0 and intact and again.tobytes() == got.tobytes()


def test_no_polygons_gives_zero_planes(L, torch_):
    rc, got, intact = device_call(L, torch_, [[], [], []], 0, 0, (7, 9))
    assert rc == 0 and intact and got.shape == (3, 7, 9) and not got.any()
    from tmlibrary_amd.image import label_planes_from_polygons
    assert not label_planes_from_polygons([[], []], 5, 5, (4, 4)).any()


def _empty_ring(points, first, plane, label):
    first[2] = first[1]


def _not_monotone(points, first, plane, label):
    first[3] = first[2] - 1


def _plane_high(points, first, plane, label):
    plane[4] = 1


def _plane_negative(points, first, plane, label):
    plane[0] = -1


def _coordinate(points, first, plane, label):
    points[7, 0] = 2 ** 24 + 40  # x_offset is 40: xs = 2^24


def _coordinate_y(points, first, plane, label):
    points[2, 1] = 2 ** 24 - 9  # y_offset is 9: ys = -2^24


@pytest.mark.parametrize("edit,word", [(_empty_ring, "empty ring"), (_not_monotone, "monotone"),
                                       (_plane_high, "out of range"),
                                       (_plane_negative, "out of range"),
                                       (_coordinate, "2^24"), (_coordinate_y, "2^24")])
def test_refusals_leave_the_output_untouched(L, torch_, edit, word):
    from tmlibrary_amd import hip
    planes = [pl.random_polygons(9, 6, (20, 24), 9, 40)]
    rc, got, intact = device_call(L, torch_, planes, 9, 40, (20, 24), edit=edit)
    assert rc == hip.TMH_EINVAL and word in L.tmh_last_error().decode(), L.tmh_last_error()
    assert intact and (got.view(np.uint8) == 0x5A).all()
    # the host form refuses the same lists and leaves its output alone
    points, first, plane, label = flat(planes)
    edit(points, first, plane, label)
    out = np.full((1, 20, 24), -7, np.int32)
    rc = L.tmh_polygon_fill(hip.ptr(points), hip.ptr(first), hip.ptr(plane), hip.ptr(label),
                            len(plane), 1, 20, 24, 9, 40, hip.ptr(out))
    assert rc == hip.TMH_EINVAL and word in L.tmh_last_error().decode(), L.tmh_last_error()
    assert (out == -7).all()


def test_device_form_refuses_overlap_and_too_many_planes(L, torch_):
    from tmlibrary_amd import hip
    planes = [pl.random_polygons(9, 6, (20, 24))]
    points, first, plane, label = flat(planes)
    d_points = torch_.from_numpy(points.reshape(-1).copy()).cuda()
    d_first = torch_.from_numpy(first).cuda()
    d_plane = torch_.from_numpy(plane).cuda()
    d_label = torch_.from_numpy(label).cuda()
    torch_.cuda.synchronize()
    at = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    rc = L.tmh_polygon_fill_device(at(d_points), at(d_first), at(d_plane), at(d_label), 6, 1, 2, 3,
                                   0, 0, at(d_points), None)
    assert rc == hip.TMH_EINVAL and "overlaps" in L.tmh_last_error().decode()
    rc = L.tmh_polygon_fill_device(at(d_points), at(d_first), at(d_plane), at(d_label), 6, 65536,
                                   2, 3, 0, 0, at(d_points), None)
    assert rc == hip.TMH_EINVAL and "65,535" in L.tmh_last_error().decode()
    assert d_points.cpu().numpy().tobytes() == points.tobytes()


def test_add_polygons(L):
    from tmlibrary_amd.workflow.jterator.handles import SegmentedObjects
    planes, y_offset, x_offset, dims = pl.CASES["stack"]
    want = pl.literal("stack")
    polygons = [[planes[t * 2 + z] for z in range(2)] for t in range(3)]
    obj = SegmentedObjects("cells", "cells")
    value = obj.add_polygons(polygons, y_offset, x_offset, dims)
    assert value is obj.value and value.dtype == np.int32 and value.shape == (96, 80, 2, 3)
    assert value.flags["C_CONTIGUOUS"]
    for t in range(3):
        for z in range(2):
            assert np.array_equal(value[:, :, z, t], want[t * 2 + z]), (t, z)
    assert [key for key, _ in obj.iter_planes()] == [(t, z) for t in range(3) for z in range(2)]
    present = sorted(set(np.unique(want).tolist()) - {0})
    assert obj.labels == present


def test_load_pipeline_input_objects(L, tmp_path):
    from tmlibrary_amd.models.file import ExperimentStore, h5lib, write_channel_image
    from tmlibrary_amd.workflow.jterator import api as japi
    from tmlibrary_amd.workflow.jterator.handles import SegmentedObjects
    h5lib()
    os.makedirs(str(tmp_path / "channel_image_files"))
    rng = np.random.default_rng(3)
    info, fid = {}, 0
    for site in (0, 1):
        for t in (0, 1, 2):
            for z in (0, 1):
                info[fid] = (0, site, 0, t, z)
                fid += 1
    store = ExperimentStore(str(tmp_path), file_info=info)
    for f in info:
        write_channel_image(store.channel_image_file(f).location,
                            rng.integers(0, 4000, (48, 64)).astype(np.uint16), gzip_level=1)
    res = dict(top=2, bottom=1, left=4, right=3)
    store.site_residues = {0: res, 1: res}
    store.site_shifts = {(0, 0): (0, 0), (1, 0): (0, 0)}
    store.site_offsets = {0: (1000, 2000), 1: (1000, 2064)}
    store.channel_names = {"dapi": 0}
    dims = (48 - 3, 64 - 7)
    store.segmentations = {}
    for site in (0, 1):
        y_offset, x_offset = store.site_offsets[site]
        for t in (0, 1, 2):
            for z in (0, 1):
                if (site, t, z) == (1, 2, 0):
                    continue  # a plane without objects has no entry
                store.segmentations[("nuclei", site, t, z)] = pl.random_polygons(
                    300 + 10 * site + 2 * t + z, 9, dims, y_offset + 2, x_offset + 4)
    pipe = japi.ImageAnalysisPipeline(1, store=store)
    plain = pipe.load_pipeline_input(1, [("dapi", False)])
    assert plain["objects"] == {} and sorted(plain["pipe"]) == ["dapi"]
    for site in (0, 1):
        st = pipe.load_pipeline_input(site, [("dapi", False)], objects=["nuclei"])
        assert sorted(st["pipe"]) == ["dapi", "nuclei"] and sorted(st["objects"]) == ["nuclei"]
        assert isinstance(st["objects"]["nuclei"], SegmentedObjects)
        if site == 1:
            assert np.array_equal(st["pipe"]["dapi"], plain["pipe"]["dapi"])
        y_offset, x_offset = store.site_offsets[site]
        want = np.zeros(dims + (2, 3), np.int32)
        for t in (0, 1, 2):
            for z in (0, 1):
                want[:, :, z, t] = pl.create_from_polygons(
                    store.segmentations.get(("nuclei", site, t, z), []), y_offset + 2,
                    x_offset + 4, dims)
        assert want.any()
        assert st["pipe"]["nuclei"].dtype == np.int32
        assert np.array_equal(st["pipe"]["nuclei"], want)
        assert np.array_equal(st["objects"]["nuclei"].value, want)
    both = pipe.load_pipeline_inputs([0, 1], [], objects=["nuclei"])
    assert [sorted(s["pipe"]) for s in both] == [["nuclei"], ["nuclei"]]
