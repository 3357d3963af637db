"""GPU: intensity measurements against tests/intensity_literal.py.

Rows equal the literal exactly, features equal it bit for bit.
"""
import ctypes as C
import os

import numpy as np
import pytest

import intensity_cases as ic
import intensity_literal as il
from util import keep  # noqa: F401

pytestmark = pytest.mark.gpu

ROW = il.ROW_DTYPE


@pytest.fixture(scope="module")
def L():
    from tmlibrary_amd import hip
    return hip.lib()


def hip_():
    from tmlibrary_amd import hip
    return hip


def table(L, keep, labels, pixels, max_label, object_rows=False, layout=None, base_offset=0,
          expect=0):
    """rows [n_planes][max_label + 1][n_channels] of labels [P][H][W] and the
    pixel buffer `pixels` (any array; plain [C][P][H][W] unless layout = (n_channels,
    channel, plane, row, pixel stride) says otherwise), read from element base_offset"""
    hip = hip_()
    labels = np.ascontiguousarray(labels, np.int32)
    P, H, W = labels.shape
    pixels = np.ascontiguousarray(pixels)
    elem = pixels.dtype.itemsize
    if layout is None:
        n_c = pixels.shape[0]
        layout = (n_c, P * H * W, H * W, W, 1)
    n_c, cs, ps, rs, xs = layout
    d_labels = keep(hip.DeviceBuffer.from_array(labels))
    d_pixels = keep(hip.DeviceBuffer.from_array(pixels))
    d_obj = keep(hip.DeviceBuffer(48)) if object_rows else None
    n_rows = P * (max_label + 1) * n_c
    guard = 64      # sentinel bytes on both sides of the rows
    d_rows = keep(hip.DeviceBuffer.from_array(np.full(n_rows * 32 + 2 * guard, 0xA5, np.uint8)))
    rc = L.tmh_intensity_table_device(d_labels, d_pixels.at(base_offset * elem), elem, P, H, W, n_c,
                                      cs, ps, rs, xs, max_label, d_obj, d_rows.at(guard), None)
    assert rc == expect, (rc, L.tmh_last_error())
    raw = d_rows.get(n_rows * 32 + 2 * guard, np.uint8)
    hip.check(L.tmh_synchronize(None))
    assert (raw[:guard] == 0xA5).all() and (raw[-guard:] == 0xA5).all()
    body = raw[guard:-guard]
    if expect != 0:
        assert (body == 0xA5).all()     # a refused call leaves the rows untouched
        return None
    return body.view(ROW).reshape(P, max_label + 1, n_c)


def features(L, keep, rows, n_groups):
    hip = hip_()
    P, n_labels, n_c = rows.shape
    d_rows = keep(hip.DeviceBuffer.from_array(rows))
    d_out = keep(hip.DeviceBuffer(n_groups * n_labels * n_c * 40))
    hip.check(L.tmh_intensity_features_device(d_rows, P, n_groups, n_labels - 1, n_c, d_out, None))
    out = d_out.get((n_groups, n_labels, n_c, 5), np.float64)
    hip.check(L.tmh_synchronize(None))
    return out


def check_against_literal(L, keep, labels, pixels, max_label=None):
    labels = np.asarray(labels, np.int32)
    if max_label is None:
        max_label = int(labels.max())
    got = table(L, keep, labels, pixels, max_label)
    want = il.table(labels, pixels, max_label)
    assert np.array_equal(got, want)
    assert il.same_bits(features(L, keep, got, labels.shape[0]),
                        il.feature_table(want, labels.shape[0]))
    return got


@pytest.mark.parametrize("dtype", [np.uint16, np.uint8])
@pytest.mark.parametrize("kind", ["cells", "checkerboard", "full", "background"])
@pytest.mark.parametrize("shape", ic.SHAPES)
def test_shapes_equal_literal(L, keep, shape, kind, dtype):
    H, W = shape
    labels = ic.label_planes(kind, H, W, seed=H + W)[None]
    if kind == "full":
        img = np.full((1, 1, H, W), np.iinfo(dtype).max, dtype)     # sum_sq at its largest
    else:
        img = ic.image((1, 1, H, W), dtype, H * W)
    got = check_against_literal(L, keep, labels, img)
    if kind == "full":
        assert got[0, 3, 0]["n"] == H * W and got[0, 3, 0]["min"] == np.iinfo(dtype).max
        assert features(L, keep, got, 1)[0, 3, 0, 4] == 0.0
    if kind == "background":
        assert got.shape == (1, 1, 1) and got[0, 0, 0]["n"] == H * W


def test_more_labels_than_the_lds_table_holds(L, keep):
    hip = hip_()
    plane = ic.many_labels_tile(700)
    assert plane.shape == ic.TILE and np.unique(plane).size == 700 > hip.INTENSITY_SLOTS
    img = ic.image((2, 1) + ic.TILE, np.uint16, 1)
    check_against_literal(L, keep, plane[None], img)


def test_labels_that_collide_beyond_the_probe_limit(L, keep):
    hip = hip_()
    plane, labels = ic.colliding_tile(hip.INTENSITY_SLOTS, hip.INTENSITY_PROBE)
    assert len(labels) == hip.INTENSITY_PROBE + 8
    assert {ic.bucket_of(l, hip.INTENSITY_SLOTS) for l in labels} == {7}
    assert set(np.unique(plane)) == set(labels) and plane.shape == ic.TILE
    img = ic.image((2, 1) + ic.TILE, np.uint16, 2)
    got = check_against_literal(L, keep, plane[None], img)
    assert (got[0, labels, 0]["n"] > 0).all()


@pytest.fixture(scope="module")
def channel_data():
    labels = np.stack([ic.cells(17, 513, 1), ic.cells(17, 513, 2)])
    img = ic.image((16, 2, 17, 513), np.uint16, 3)
    max_label = int(labels.max())
    single = [il.table(labels, img[c:c + 1], max_label) for c in range(16)]
    return labels, img, max_label, single


@pytest.mark.parametrize("n_channels", [1, 2, 3, 4, 5, 16])
def test_channels_in_one_call_equal_one_channel_calls(L, keep, channel_data, n_channels):
    labels, img, max_label, single = channel_data
    got = table(L, keep, labels, img[:n_channels], max_label)
    for c in range(n_channels):
        assert np.array_equal(got[:, :, c], single[c][:, :, 0]), c
        if n_channels in (5, 16) and c % 4 == 0:
            one = table(L, keep, labels, img[c:c + 1], max_label)
            assert one.tobytes() == np.ascontiguousarray(got[:, :, c:c + 1]).tobytes()


def test_interleaved_stack_layout_and_odd_base(L, keep):
    """[2 sites][h][w][3 slots] as the channel stack writes it: slot 1 of both
    sites through strides; the same pixels contiguous from a base pointer one
    element in; both give the same bytes."""
    h, w = 33, 130
    stack = ic.image((2, h, w, 3), np.uint16, 4)
    labels = np.stack([ic.cells(h, w, 5), ic.checkerboard(h, w)])
    max_label = int(labels.max())
    strided = table(L, keep, labels, stack, max_label, layout=(1, 0, h * w * 3, w * 3, 3),
                    base_offset=1)
    plain = np.ascontiguousarray(stack[:, :, :, 1])[None]
    assert np.array_equal(strided, il.table(labels, plain, max_label))
    shifted = np.concatenate([np.zeros(1, np.uint16), plain.reshape(-1)])
    contiguous = table(L, keep, labels, shifted, max_label, layout=(1, 0, h * w, w, 1),
                       base_offset=1)
    assert contiguous.tobytes() == strided.tobytes()
    # all three slots as three channels of one call: channel stride 1
    three = table(L, keep, labels, stack, max_label, layout=(3, 1, h * w * 3, w * 3, 3))
    for c in range(3):
        want = il.table(labels, np.ascontiguousarray(stack[:, :, :, c])[None], max_label)
        assert np.array_equal(three[:, :, c:c + 1], want)


def test_label_above_max_label(L, keep):
    hip = hip_()
    labels = ic.cells(17, 513, 7)[None].copy()
    top = int(labels.max())
    labels[0, 5, 100:140] = top + 50
    labels[0, 16, 512] = top + 1
    img = ic.image((2, 1, 17, 513), np.uint16, 8)
    # without the object table's rows the call checks the range itself
    assert table(L, keep, labels, img, top, expect=hip.TMH_EINVAL) is None
    assert b"above max_label" in L.tmh_last_error()
    bad = labels.copy()
    bad[0, 0, 0] = -1
    assert table(L, keep, bad, img, top + 50, expect=hip.TMH_EINVAL) is None
    assert b"negative label" in L.tmh_last_error()
    # with them the range counts as checked: the kernel skips the label on its own
    got = table(L, keep, labels, img, top, object_rows=True)
    assert np.array_equal(got, il.table(labels, img, top))


def test_finalize_entry_on_extreme_rows(L, keep):
    hip = hip_()
    for rows, n_groups in ic.finalize_cases():
        want = il.feature_table(rows, n_groups)
        assert il.same_bits(features(L, keep, rows, n_groups), want)
        out = np.zeros(want.shape, np.float64)
        hip.check(L.tmh_intensity_features(hip.ptr(np.ascontiguousarray(rows)), rows.shape[0],
                                           n_groups, rows.shape[1] - 1, rows.shape[2],
                                           hip.ptr(out)))
        assert il.same_bits(out, want)
    extreme = features(L, keep, *ic.finalize_cases()[0])[0, :, 0]
    assert extreme[0, 4] == 0.0 and extreme[1, 4] > 0.0 and np.isnan(extreme[5]).all()


def test_refusals_by_name(L, keep):
    hip = hip_()
    d = keep(hip.DeviceBuffer(4 * 8 * 8 + 2 * 8 * 8 + 64 * 32))
    lab, pix, rows = d.at(0), d.at(256), d.at(384)

    def call(n_planes=1, elem=2, n_c=1, strides=(64, 64, 8, 1), rows=rows, max_label=0):
        return L.tmh_intensity_table_device(lab, pix, elem, n_planes, 8, 8, n_c, *strides,
                                            max_label, lab, rows, None)
    for kwargs, word in ((dict(n_c=0), b"n_channels"), (dict(n_c=17), b"n_channels"),
                         (dict(elem=4), b"elem_bytes"), (dict(elem=0), b"elem_bytes"),
                         (dict(n_planes=65536), b"65,535"),
                         (dict(strides=(64, 64, -8, 1)), b"negative"),
                         (dict(strides=(-1, 64, 8, 1)), b"negative"),
                         (dict(rows=pix), b"overlaps"), (dict(rows=lab), b"overlaps"),
                         (dict(max_label=-1), b"max_label")):
        assert call(**kwargs) == hip.TMH_EINVAL, kwargs
        assert word in L.tmh_last_error(), (kwargs, L.tmh_last_error())
    assert call(n_planes=0) == 0
    assert L.tmh_intensity_features_device(rows, 3, 2, 0, 1, pix, None) == hip.TMH_EINVAL
    assert b"divide" in L.tmh_last_error()
    assert L.tmh_intensity_features_device(rows, 0, 0, 0, 1, None, None) == 0


def test_host_form_and_row_capacity(L):
    hip = hip_()
    labels = np.stack([ic.cells(17, 65, 1), ic.cells(17, 65, 2)])
    img = ic.image((2, 2, 17, 65), np.uint8, 3)
    top = int(labels.max())
    mx = C.c_int32(-7)
    rows = np.full((2, top + 1, 2), 0, ROW)
    rows["n"] = -1
    rc = L.tmh_intensity_table(hip.ptr(labels), hip.ptr(img), 1, 2, 17, 65, 2, C.byref(mx),
                               hip.ptr(rows), rows.size - 1)
    assert rc == hip.TMH_EINVAL and mx.value == top and (rows["n"] == -1).all()
    hip.check(L.tmh_intensity_table(hip.ptr(labels), hip.ptr(img), 1, 2, 17, 65, 2, C.byref(mx),
                                    hip.ptr(rows), rows.size))
    assert np.array_equal(rows, il.table(labels, img, top))


def test_two_calls_identical_bytes(L, keep):
    labels = np.stack([ic.cells(33, 1030, 3), ic.checkerboard(33, 1030)])
    img = ic.image((4, 2, 33, 1030), np.uint16, 9)
    top = int(labels.max())
    a = table(L, keep, labels, img, top)
    b = table(L, keep, labels, img, top)
    assert a.tobytes() == b.tobytes()
    assert features(L, keep, a, 2).tobytes() == features(L, keep, b, 2).tobytes()


def literal_frames(labels4, image4):
    """per time point (present labels, features [n][5]) of (h, w, z, t) arrays"""
    planes = np.ascontiguousarray(labels4.transpose(3, 2, 0, 1))
    n_t, n_z = planes.shape[:2]
    planes = planes.reshape((n_t * n_z,) + planes.shape[2:])
    img = np.ascontiguousarray(image4.transpose(3, 2, 0, 1)).reshape((1,) + planes.shape)
    feats = il.feature_table(il.table(planes, img, int(planes.max())), n_t)
    out = []
    for t in range(n_t):
        present = np.unique(labels4[..., t][labels4[..., t] > 0])
        out.append((present, feats[t, present, 0]))
    return out


def check_measurement(m, channel, labels4, image4):
    from tmlibrary_amd.workflow.jterator.measure import feature_names
    assert m.channel_ref == channel and m.type == "Measurement"
    want = literal_frames(labels4, image4)
    assert len(m.value) == len(want)
    for frame, (present, feats) in zip(m.value, want):
        assert frame.columns.tolist() == feature_names(channel)
        assert np.array_equal(frame.index.values, present)
        assert il.same_bits(frame.values, feats)


def test_z_planes_of_a_time_point_are_one_object(L):
    import torch
    from tmlibrary_amd.workflow.jterator.handles import SegmentedObjects
    from tmlibrary_amd.workflow.jterator.measure import measure_intensity
    h, w = 20, 70
    labels = np.zeros((h, w, 3, 2), np.int32)
    for t in range(2):
        base = ic.cells(h, w, 11 + t)
        for z in range(3):
            labels[:, :, z, t] = np.roll(base, z, axis=1)
    labels[:, :, 1, 0][labels[:, :, 1, 0] == 2] = 0      # label 2 absent from one z-plane
    labels[:, :, :, 1][labels[:, :, :, 1] == 3] = 0      # label 3 absent from a time point
    images = {"dapi": ic.image((h, w, 3, 2), np.uint16, 1), "gfp-2": ic.image((h, w, 3, 2),
                                                                             np.uint16, 2)}
    got = measure_intensity(labels, images)
    assert [m.name for m in got] == ["Intensity_dapi", "Intensity_gfp-2"]
    for m, (name, img) in zip(got, images.items()):
        check_measurement(m, name, labels, img)
    assert 3 in got[0].value[0].index and 3 not in got[0].value[1].index
    # device tensors of the same layout, and a SegmentedObjects that has its table
    obj = SegmentedObjects("cells", "cells")
    obj.value = labels
    obj.object_tables()
    dev = {k: torch.from_numpy(v.view(np.int16)).cuda() for k, v in images.items()}
    again = measure_intensity(obj, dev)
    for a, b in zip(got, again):
        assert b.objects == "cells"
        for fa, fb in zip(a.value, b.value):
            assert fa.equals(fb)
        obj.add_measurement(b)
    assert obj.measurements[0].shape[1] == 10
    # uint8, 2-D
    flat = measure_intensity(labels[:, :, 0, 0], {"c": ic.image((h, w), np.uint8, 3)})
    check_measurement(flat[0], "c", labels[:, :, :1, :1], ic.image((h, w), np.uint8, 3)
                      [:, :, None, None])


def test_end_to_end_from_files_to_clustering(L, tmp_path):
    """load_pipeline_inputs -> label planes -> measure_intensity on the device
    stack -> add_measurement -> save_measurements -> Clustering labels every object"""
    import torch
    import polygons_literal as pl
    from tmlibrary_amd.models.file import ExperimentStore, h5lib, write_channel_image
    from tmlibrary_amd.tools.base import FeatureStore
    from tmlibrary_amd.tools.clustering import Clustering
    from tmlibrary_amd.workflow.jterator import api as japi
    from tmlibrary_amd.workflow.jterator.measure import measure_intensity, save_measurements
    h5lib()
    os.makedirs(str(tmp_path / "channel_image_files"))
    rng = np.random.default_rng(3)
    info, fid = {}, 0
    for channel in (0, 1):
        for site in (0, 1):
            for t in (0, 1):
                info[fid] = (channel, site, 0, t, 0)
                fid += 1
    store = ExperimentStore(str(tmp_path), file_info=info)
    for f in info:
        write_channel_image(store.channel_image_file(f).location,
                            rng.integers(0, 60000, (48, 64)).astype(np.uint16), gzip_level=1)
    store.channel_names = {"dapi": 0, "gfp": 1}
    store.site_offsets = {0: (1000, 2000), 1: (1000, 2064)}
    dims = (48, 64)
    store.segmentations = {}
    for site in (0, 1):
        y_offset, x_offset = store.site_offsets[site]
        rings = pl.random_polygons(300 + site, 9, dims, y_offset, x_offset)
        for t in (0, 1):
            store.segmentations[("nuclei", site, t, 0)] = rings
    pipe = japi.ImageAnalysisPipeline(1, store=store)
    sites = pipe.load_pipeline_inputs([0, 1], [("dapi", False), ("gfp", False)],
                                      objects=["nuclei"])
    # the channel stack as it lies on the device: [site][h][w][slot], slot = t here
    # both channels in one allocation, so all of it is read in place
    both = torch.from_numpy(np.stack([np.stack([st["pipe"][name] for st in sites])
                                      for name in ("dapi", "gfp")]).view(np.int16)).cuda()
    stacks = {"dapi": both[0], "gfp": both[1]}
    features = FeatureStore()
    n_objects = 0
    for k, st in enumerate(sites):
        obj = st["objects"]["nuclei"]
        assert obj.value.shape == dims + (1, 2) and obj.labels
        images = {name: stacks[name][k].unsqueeze(2) for name in stacks}     # (h, w, 1, t) views
        for m in measure_intensity(obj, images):
            check_measurement(m, m.channel_ref, obj.value,
                              st["pipe"][m.channel_ref][:, :, None, :])
            obj.add_measurement(m)
        assert obj.measurements[0].shape == (len(obj.labels), 10)
        ids = save_measurements(features, obj, st["site_id"])
        assert len(ids) == 2 * len(obj.labels)
        n_objects += len(ids)
    names = obj.measurements[0].columns.tolist()
    table = features.load_feature_values("nuclei", names)
    assert table.values.shape == (n_objects, 10) and np.isfinite(table.values).all()
    first = sites[0]["objects"]["nuclei"].measurements[0].round(6).values
    assert np.array_equal(table.values[:len(first)], first)
    tool = Clustering(1, store=features)
    tool.process_request(1, {"chosen_object_type": "nuclei", "selected_features": names,
                             "options": {"k": 2, "method": "kmeans"}})
    result = features.results[1]["values"]
    assert sorted(result) == list(range(1, n_objects + 1))
    assert set(result.values()) <= {0, 1}
