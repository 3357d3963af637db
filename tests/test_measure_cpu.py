"""CPU: the intensity rule, the finalize core and the handles.

tests/intensity_literal.py states the rule in numpy and Python ints;
tmlibrary_amd/csrc/intensity_core.h is the code the finalize kernel runs,
compiled here with g++ through tests/intensity_host.cpp.
"""
import collections
import logging
import math
import os
import statistics
import subprocess

import numpy as np
import pandas as pd
import pytest

import intensity_cases as ic
import intensity_literal as il
from util import REPO

HARNESS = os.path.join(REPO, "tests", "intensity_host.cpp")
FLAGS = ["-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas"]


# ---------------------------------------------------------------- the rule

def std_cases():
    """32 value lists: random 16-bit data, two values at the top of the range,
    one differing pixel among 100,000, a narrow range"""
    out = []
    for seed in range(8):
        rng = np.random.default_rng(seed)
        out.append(rng.integers(0, 65536, 1000 + 37 * seed))
        out.append(rng.integers(65534, 65536, 500 + seed))
        v = np.full(100000, 40000 + seed)
        v[rng.integers(0, v.size)] += 1
        out.append(v)
        out.append(rng.integers(30000, 30004, 2000 + seed))
    return [[int(x) for x in v] for v in out]


def test_literal_equals_numpy_exactly():
    for seed, dtype in enumerate((np.uint16, np.uint8, np.uint16)):
        labels = ic.cells(33, 70, seed)
        img = ic.image((33, 70), dtype, 10 + seed)
        rows = il.plane_rows(labels, img, int(labels.max()))
        for l in range(int(labels.max()) + 1):
            v = img[labels == l]
            f = il.features(il.as_ints(rows[l]))
            if v.size == 0:
                assert all(math.isnan(x) for x in f)
                continue
            want = [np.max(v), np.mean(v), np.min(v), np.sum(v, dtype=np.uint64)]
            assert [float(x) for x in want] == f[:4]
            assert rows[l]["n"] == v.size


def test_literal_std_within_4_ulp_of_pstdev():
    """The rule rounds three times (0.25 + 0.5 + 0.5 ulp of the result: the
    conversion's half ulp is halved by the square root), pstdev rounds an
    exact fraction and takes one sqrt (0.25 + 0.5): 2 ulp together, doubled
    for a binade edge between the two.  np.std is a cross-check only."""
    cases = std_cases()
    assert len(cases) == 32
    worst = 0.0
    for v in cases:
        got = il.features(il.row_of(v))[4]
        want = statistics.pstdev(v)
        ulps = abs(got - want) / math.ulp(want) if want else abs(got)
        worst = max(worst, ulps)
        assert ulps <= 4, (ulps, got, want)
        assert abs(got - float(np.std(np.asarray(v)))) <= 1e-12 * max(want, 1e-300) + 1e-9
    print("worst distance to pstdev: %.2f ulp" % worst)


def test_constant_object_has_std_zero():
    assert il.features(il.row_of([65535] * 1000))[4] == 0.0
    assert il.features(ic.EXTREME_ROWS[0])[4] == 0.0


# ------------------------------------------------- the finalize core on the host

def run_host(exe, tmp_path, rows, n_groups):
    src, dst = str(tmp_path / "in"), str(tmp_path / "out")
    n_planes, n_labels, n_channels = rows.shape
    with open(src, "wb") as f:
        f.write(np.array([n_groups, n_planes // n_groups, n_labels * n_channels],
                         np.int64).tobytes())
        f.write(np.ascontiguousarray(rows).tobytes())
    subprocess.run([exe, src, dst], check=True)
    return np.fromfile(dst, np.float64).reshape(n_groups, n_labels, n_channels, 5)


def image_rows():
    """rows of a real image: 3 z x 2 t planes, 2 channels, one label absent from a plane"""
    labels = np.stack([ic.cells(20, 70, s) for s in range(6)])
    labels[1][labels[1] == 2] = 0
    images = np.stack([ic.image((6, 20, 70), np.uint16, 5), ic.image((6, 20, 70), np.uint16, 6)])
    return il.table(labels, images, int(labels.max()))


def check_host(exe, tmp_path):
    for rows, n_groups in ic.finalize_cases() + [(image_rows(), 2)]:
        got = run_host(exe, tmp_path, rows, n_groups)
        assert il.same_bits(got, il.feature_table(rows, n_groups))
    extreme = run_host(exe, tmp_path, *ic.finalize_cases()[0])[0, :, 0]
    assert extreme[0, 4] == 0.0 and extreme[0, 1] == 65535.0
    assert extreme[1, 4] > 0.0 and extreme[4].tolist() == [12345.0, 12345.0, 12345.0, 12345.0, 0.0]
    assert np.isnan(extreme[5]).all()
    merged = run_host(exe, tmp_path, *ic.finalize_cases()[1])[0, :, 0]
    assert merged[0].tolist()[:4] == [65535.0, (5 + 9 + 70 + 3 + 65535) / 5, 3.0, 65622.0]
    assert merged[1, 2] == 2.0 and np.isnan(merged[2]).all() and merged[3, 2] == 0.0


def test_host_core_equals_literal(tmp_path):
    exe = str(tmp_path / "intensity_host")
    subprocess.run(["g++", "-O2"] + FLAGS + ["-o", exe, HARNESS], check=True, capture_output=True)
    check_host(exe, tmp_path)
    # a file that ends early is refused, not read past
    src = str(tmp_path / "short")
    with open(src, "wb") as f:
        f.write(np.array([1, 1, 4], np.int64).tobytes())
        f.write(bytes(32 * 3))
    assert subprocess.run([exe, src, str(tmp_path / "o")]).returncode == 6


def test_host_core_under_sanitizers(tmp_path):
    san = str(tmp_path / "intensity_host_san")
    r = subprocess.run(["g++", "-O1", "-g", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all"] + FLAGS + ["-o", san, HARNESS],
                       capture_output=True, text=True)
    if r.returncode != 0 and ("asan" in r.stderr or "ubsan" in r.stderr or "sanitize" in r.stderr):
        pytest.skip("g++ here lacks the sanitizer runtimes: " + r.stderr.strip().splitlines()[-1])
    assert r.returncode == 0, r.stderr
    check_host(san, tmp_path)


def test_u128_conversion_rounds_once():
    """The sticky-bit form the core uses, restated on Python ints, equals
    float(int) on values up to 94 bits, ties and near-ties included; the
    two-halves form, which rounds twice, does not."""
    rng = np.random.default_rng(1)
    values = [(1 << 64) + (1 << 11) + 1, (1 << 64) + (1 << 11), (1 << 64) + (3 << 11),
              (1 << 93) + (1 << 40) + 1, (1 << 94) - 1]
    for _ in range(2000):
        bits = int(rng.integers(65, 95))
        values.append((1 << (bits - 1)) | int(rng.integers(0, 1 << 62)) << max(0, bits - 63)
                      | int(rng.integers(0, 2)))
    twice_differs = 0
    for v in values:
        drop = v.bit_length() - 64
        top = (v >> drop) | (1 if v & ((1 << drop) - 1) else 0)
        assert math.ldexp(float(top), drop) == float(v), v
        hi, lo = v >> 64, v & ((1 << 64) - 1)
        twice_differs += float(hi) * 2.0 ** 64 + float(lo) != float(v)
    assert twice_differs > 0


# ------------------------------------------------------------------ ABI

def test_row_dtype_and_constants_match_the_binding():
    from tmlibrary_amd import hip
    assert hip.INTENSITY_ROW_DTYPE == il.ROW_DTYPE
    assert hip.INTENSITY_FEATURES == il.FEATURES
    text = open(os.path.join(REPO, "include", "tmhip.h")).read()
    for name in ("SLOTS", "PROBE", "PASS_CHANNELS", "MAX_CHANNELS"):
        assert "#define TMH_INTENSITY_%s %d\n" % (name, getattr(hip, "INTENSITY_" + name)) in text
    lib = hip.load_library()
    for name in ("tmh_intensity_table", "tmh_intensity_features"):
        for full in (name, name + "_device"):
            assert full in hip.SIGNATURES and full + "(" in text and hasattr(lib, full)
    labels = ic.same_bucket_labels(7, 4, hip.INTENSITY_SLOTS)
    assert all(ic.bucket_of(l, hip.INTENSITY_SLOTS) == 7 for l in labels)


# -------------------------------------------------------------- handles

def objects_with_labels(labels, key="cells"):
    """a SegmentedObjects whose object table is set by hand (no GPU here)"""
    from tmlibrary_amd import hip
    from tmlibrary_amd.workflow.jterator.handles import SegmentedObjects
    obj = SegmentedObjects(key, key)
    obj.value = np.zeros((4, 4), np.int32)
    rows = np.zeros(max(labels) + 1, hip.OBJECT_ROW_DTYPE)
    rows["n"][list(labels)] = 1
    obj._tables = collections.OrderedDict([((0, 0), rows)])
    return obj


def frame(index, **columns):
    return pd.DataFrame(columns, index=pd.Index(index))


def test_measurement_handle_messages():
    from tmlibrary_amd.workflow.jterator.handles import Measurement
    m = Measurement("feats", "cells", "cells", channel_ref="dapi", help="h")
    assert m.type == "Measurement"
    assert m.to_dict() == {"name": "feats", "objects": "cells", "objects_ref": "cells",
                           "channel_ref": "dapi", "type": "Measurement", "help": "h"}
    assert str(m) == "<Measurement(name='feats', objects='cells')>"
    with pytest.raises(TypeError, match='Value of key "feats" must have type list.'):
        m.value = frame([1], a=[1.0])
    with pytest.raises(TypeError, match='Elements of returned value of "feats" must have type '
                                        'pandas.DataFrame.'):
        m.value = [np.zeros(3)]
    with pytest.raises(ValueError, match='Feature name "a b" must only contain alphanumerical '
                                         'characters or underscores or hyphens'):
        m.value = [frame([1], **{"a b": [1.0]})]
    m.value = [frame([1], **{"Intensity_mean_dapi-2": [1.0]})]
    assert m.value[0].shape == (1, 1)
    for bad in ((1, "c", None), ("c", 2, None), ("c", "c", 3)):
        with pytest.raises(TypeError):
            Measurement("feats", *bad)
    assert Measurement("f", "a", "b").channel_ref is None


def test_add_measurement_pads_removes_and_refuses(caplog):
    from tmlibrary_amd.workflow.jterator.handles import Measurement
    obj = objects_with_labels([1, 2, 4])
    assert obj.labels == [1, 2, 4]
    assert len(obj.measurements) == 1 and obj.measurements[0].empty
    with pytest.raises(TypeError, match='Argument "measurement" must have type '
                                        'tmlib.workflow.jterator.handles.Measurement.'):
        obj.add_measurement(frame([1], a=[1.0]))
    m = Measurement("m", "cells", "cells")
    # a missing label is padded with NaN, the caller's frame stays as it was
    short = frame([4, 1], a=[4.0, 1.0])
    m.value = [short]
    with caplog.at_level(logging.WARNING):
        obj.add_measurement(m)
    assert "add NaN values for missing object #2" in caplog.text
    assert short.index.tolist() == [4, 1] and short.shape == (2, 1)
    got = obj.measurements[0]
    assert got.index.tolist() == [1, 2, 4]
    assert got["a"].tolist()[0] == 1.0 and math.isnan(got["a"].tolist()[1])
    # duplicates: the first is kept
    m2 = Measurement("m2", "cells", "cells")
    m2.value = [frame([1, 2, 2, 4], b=[1.0, 2.0, 22.0, 4.0])]
    obj.add_measurement(m2)
    assert obj.measurements[0]["b"].tolist() == [1.0, 2.0, 4.0]
    # unknown labels are removed
    m3 = Measurement("m3", "cells", "cells")
    extra = frame([1, 2, 3, 4], c=[1.0, 2.0, 3.0, 4.0])
    m3.value = [extra]
    obj.add_measurement(m3)
    assert extra.shape == (4, 1)
    assert obj.measurements[0].columns.tolist() == ["a", "b", "c"]
    assert obj.measurements[0]["c"].tolist() == [1.0, 2.0, 4.0]
    # the two refusals
    m4 = Measurement("m4", "cells", "cells")
    m4.value = [frame([1, 2, 5], d=[1.0, 2.0, 5.0])]
    with pytest.raises(ValueError, match='Labels of objects for "m4" at time point 0 do not match!'):
        obj.add_measurement(m4)
    m5 = Measurement("m5", "cells", "cells")
    m5.value = [pd.DataFrame(np.zeros((3, 2)), index=[1, 2, 4], columns=["e", "e"])]
    with pytest.raises(ValueError, match='Column names of "m5" at time point 0 must be unique.'):
        obj.add_measurement(m5)


def test_measurements_setter_and_time_points():
    from tmlibrary_amd.workflow.jterator.handles import Measurement
    obj = objects_with_labels([1, 2])
    with pytest.raises(TypeError, match='Argument "measurements" must have type list.'):
        obj.measurements = frame([1], a=[1.0])
    with pytest.raises(TypeError, match='Items of argument "measurements" must have type '
                                        'pandas.DataFrame.'):
        obj.measurements = [1]
    obj.measurements = [frame([1, 2], a=[1.0, 2.0]), frame([1, 2], a=[3.0, 4.0])]
    m = Measurement("m", "cells", "cells")
    m.value = [frame([1, 2], b=[5.0, 6.0]), frame([1, 2], b=[7.0, 8.0])]
    obj.add_measurement(m)
    got = obj.measurements
    assert len(got) == 2
    assert got[0].columns.tolist() == ["a", "b"] and got[1]["b"].tolist() == [7.0, 8.0]
    obj.measurements = []
    assert obj.measurements[0].empty


def test_save_measurements_rounds_and_issues_ids(caplog):
    from tmlibrary_amd.tools.base import FeatureStore
    from tmlibrary_amd.workflow.jterator.measure import save_measurements
    store = FeatureStore()
    obj = objects_with_labels([1, 2], key="nuclei")
    obj.measurements = [frame([1, 2], a=[1.23456749, 2.5], b=[0.0000004, 7.0]),
                        pd.DataFrame(),
                        frame([1, 2], a=[3.0, 4.0], b=[5.0, 6.0])]
    with caplog.at_level(logging.WARNING):
        ids = save_measurements(store, obj, site_id=9)
    assert "empty measurement at time point 1" in caplog.text
    assert ids == {(9, 0, 1): 1, (9, 0, 2): 2, (9, 2, 1): 3, (9, 2, 2): 4}
    table = store.load_feature_values("nuclei", ["a", "b"])
    assert table.index.tolist() == [1, 2, 3, 4]
    assert table.values.tolist() == [[1.234567, 0.0], [2.5, 7.0], [3.0, 5.0], [4.0, 6.0]]
    # a second site goes on above the ids there are
    more = save_measurements(store, obj, site_id=10)
    assert sorted(more.values()) == [5, 6, 7, 8]


def test_append_mapobjects_refusals():
    from tmlibrary_amd.tools.base import FeatureStore
    store = FeatureStore()
    store.add_mapobject_type("cells", [10, 3], ["a", "b"], [[1.0, 2.0], [3.0, 4.0]])
    ids = store.append_mapobjects("cells", ["a", "b"], [[5.0, 6.0]])
    assert ids.tolist() == [11]
    assert store.load_feature_values("cells", ["b"], [3, 10, 11]).values.tolist() == \
        [[4.0], [2.0], [6.0]]
    with pytest.raises(ValueError, match="Feature names differ"):
        store.append_mapobjects("cells", ["a", "c"], [[5.0, 6.0]])
    with pytest.raises(ValueError, match="shape"):
        store.append_mapobjects("cells", ["a", "b"], [[5.0]])
    assert store.load_feature_values("cells", ["a"]).values.shape == (3, 1)
    assert store.append_mapobjects("fresh", ["x"], np.zeros((0, 1))).size == 0
    assert store.append_mapobjects("fresh", ["x"], [[1.0], [2.0]]).tolist() == [1, 2]


def test_measure_intensity_refuses_before_any_launch():
    """shape, dtype and name mismatches raise before the library is asked for
    a device (there is none here)"""
    from tmlibrary_amd.workflow.jterator.measure import feature_names, measure_intensity
    labels = np.zeros((4, 5), np.int32)
    ok = np.zeros((4, 5), np.uint16)
    assert feature_names("dapi") == ["Intensity_max_dapi", "Intensity_mean_dapi",
                                     "Intensity_min_dapi", "Intensity_sum_dapi",
                                     "Intensity_std_dapi"]
    with pytest.raises(TypeError, match="int32"):
        measure_intensity(labels.astype(np.int64), {"dapi": ok})
    with pytest.raises(TypeError, match="only uint8 and uint16"):
        measure_intensity(labels, {"dapi": ok.astype(np.float32)})
    with pytest.raises(TypeError, match="only uint8 and uint16"):
        measure_intensity(labels, {"dapi": ok.astype(np.int32)})
    with pytest.raises(TypeError, match="share one data type"):
        measure_intensity(labels, {"a": ok, "b": ok.astype(np.uint8)})
    with pytest.raises(ValueError, match="shape"):
        measure_intensity(labels, {"dapi": np.zeros((4, 6), np.uint16)})
    with pytest.raises(ValueError, match='Feature name "Intensity_max_da pi" must only contain'):
        measure_intensity(labels, {"da pi": ok})
    with pytest.raises(TypeError, match="non-empty dict"):
        measure_intensity(labels, {})
    with pytest.raises(ValueError, match="at most 16"):
        measure_intensity(labels, {"c%d" % i: ok for i in range(17)})
    with pytest.raises(ValueError, match="negative label"):
        measure_intensity(labels - 1, {"dapi": ok})
