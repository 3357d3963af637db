"""CPU: the fill rule of create_from_polygons and the kernel's core.

tests/polygons_literal.py restates skimage.draw.polygon of scikit-image 0.13.0
in plain loops; tmlibrary_amd/csrc/polygon_core.h is the code the polygon
kernels run, compiled here with g++ through tests/polygon_host.cpp.  Neither
library is installed, so the literal is held to four hand anchors, to the
properties any even-odd fill has, and to matplotlib's point-in-path test on
every pixel that lies on no edge; the core is then held to the literal on the
GPU tests' cases.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import polygons_literal as pl
from util import REPO

HARNESS = os.path.join(REPO, "tests", "polygon_host.cpp")
FLAGS = ["-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas"]


def write_cases(path, names):
    with open(path, "wb") as f:
        n = sum(len(pl.CASES[name][0]) for name in names)
        f.write(np.array([n], np.int32).tobytes())
        for name in names:
            planes, y_offset, x_offset, dims = pl.CASES[name]
            for polygons in planes:
                f.write(np.array([dims[0], dims[1], len(polygons)], np.int32).tobytes())
                f.write(np.array([y_offset, x_offset], np.int64).tobytes())
                for label, ring in polygons:
                    f.write(np.array([label, len(ring)], np.int64).astype(np.int32).tobytes())
                    f.write(np.ascontiguousarray(ring, dtype=np.int32).tobytes())


def run_host(exe, tmp_path, names):
    """name -> int32 [n_planes, H, W] by the host build of the core"""
    src, dst = str(tmp_path / "in"), str(tmp_path / "out")
    write_cases(src, names)
    subprocess.run([exe, src, dst], check=True)
    raw, at, out = open(dst, "rb").read(), 0, {}
    for name in names:
        planes, _, _, (H, W) = pl.CASES[name]
        out[name] = np.frombuffer(raw, np.int32, len(planes) * H * W, at).reshape(len(planes), H, W)
        at += 4 * len(planes) * H * W
    assert at == len(raw)
    return out


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("polygon") / "polygon_host")
    subprocess.run(["g++", "-O2"] + FLAGS + ["-o", out, HARNESS], check=True, capture_output=True)
    return out


def check_anchors(result_of):
    for k, (_, shape, pixels) in enumerate(pl.ANCHORS):
        got = result_of("anchor%d" % k)
        assert got.dtype == np.int32 and got.shape == (1,) + shape
        assert np.array_equal(got[0], pl.anchor_plane(shape, pixels)), k


def check_properties(result_of):
    """What the rule gives whatever the code: see the cases' comments."""
    for name in ("one_vertex", "two_vertices", "outside"):
        assert not result_of(name).any(), name
    for name in ("cross_left", "cross_right", "cross_top", "cross_bottom", "cross_all"):
        assert result_of(name).any(), name
    # the triangle shifted over an edge is the unshifted one, clipped
    (ring,) = [r for _, r in pl.CASES["cross_left"][0][0]]
    whole = pl.create_from_polygons([(7, ring + np.array([4, 0], np.int32))], 0, 0, (16, 24))
    assert np.array_equal(result_of("cross_left")[0][:, :16], whole[:, 4:20])
    assert np.array_equal(result_of("unclosed"), result_of("closed"))
    assert np.array_equal(result_of("unclosed"), result_of("reversed"))
    # the bow-tie (1,1) (11,9) (11,1) (1,9) crosses itself at (6, 5): even-odd
    # fills the two triangles left and right of it and neither above nor below
    bow = result_of("bowtie")[0]
    assert bow[5, 2] == 4 and bow[5, 9] == 4 and bow[2, 6] == 0 and bow[8, 6] == 0
    # the later ring of a list wins where two overlap
    ab, ba = result_of("overlap_ab")[0], result_of("overlap_ba")[0]
    both = (ab != 0) & (ab != ba)
    assert both.sum() > 50 and (ab[both] == 22).all() and (ba[both] == 11).all()
    assert np.array_equal(ab != 0, ba != 0)


def test_literal_anchors():
    check_anchors(pl.literal)


def test_host_core_anchors(exe, tmp_path):
    got = run_host(exe, tmp_path, ["anchor%d" % k for k in range(4)])
    check_anchors(got.__getitem__)


def test_literal_properties():
    check_properties(pl.literal)


def test_host_core_properties(exe, tmp_path):
    got = run_host(exe, tmp_path, list(pl.CASES))
    check_properties(got.__getitem__)


def test_host_core_equals_literal(exe, tmp_path):
    names = list(pl.CASES)
    got = run_host(exe, tmp_path, names)
    for name in names:
        assert got[name].tobytes() == pl.literal(name).tobytes(), name


def test_cases_take_both_routes():
    """The cases named for a side of the LDS threshold lie on it."""
    from tmlibrary_amd import hip

    def words(name):
        planes, y_offset, x_offset, dims = pl.CASES[name]
        return pl.box_words(planes[0][0][1], y_offset, x_offset, dims)

    assert hip.POLYGON_LDS_WORDS == 512
    assert words("threshold_below") == hip.POLYGON_LDS_WORDS
    assert words("threshold_above") == hip.POLYGON_LDS_WORDS + 1
    for w in (63, 64, 65, 129):
        assert words("width%d_lds" % w) == 12 * ((w + 63) // 64) <= hip.POLYGON_LDS_WORDS
        assert words("width%d_mem" % w) == 600 * ((w + 63) // 64) > hip.POLYGON_LDS_WORDS


def on_an_edge(pts, x, y):
    n = len(pts)
    for i in range(n):
        (x0, y0), (x1, y1) = pts[i], pts[(i + 1) % n]
        if (x1 - x0) * (y - y0) == (y1 - y0) * (x - x0) and min(x0, x1) <= x <= max(x0, x1) \
                and min(y0, y1) <= y <= max(y0, y1):
            return True
    return False


def test_literal_equals_matplotlib_off_the_edges():
    """40 random stars on a 28 x 30 plane, every pixel of the plane per star:
    where the pixel lies on no edge, the literal and
    matplotlib.path.Path.contains_point agree exactly.  Pixels on an edge are
    where an edge-inclusive and this edge-exclusive test may differ; they are
    left out and may be at most 5 % of the tested pixels."""
    from matplotlib.path import Path

    rng = np.random.default_rng(0)
    H, W = 28, 30
    tested = skipped = inside = 0
    for _ in range(40):
        pts = pl.star(rng, rng.uniform(4, H - 4), rng.uniform(4, W - 4), rng.uniform(4, 13),
                      int(rng.integers(3, 10)))
        plane = np.zeros((H, W), np.int32)
        pl.fill_ring(plane, 1, [float(p[0]) for p in pts], [float(p[1]) for p in pts])
        path = Path(np.array(pts + pts[:1], float), closed=True)
        for r in range(H):
            for c in range(W):
                tested += 1
                if on_an_edge(pts, c, r):
                    skipped += 1
                    continue
                assert bool(plane[r, c]) == bool(path.contains_point((c, r))), (pts, r, c)
                inside += int(plane[r, c])
    assert tested == 40 * H * W
    assert skipped <= 0.05 * tested, (skipped, tested)
    assert inside > 2000


def test_case_list_under_sanitizers(tmp_path):
    """The stand-alone harness built with -fsanitize=address,undefined: the bit
    rows and the planes are heap blocks of their exact size, so a toggle or a
    pixel written outside a box ends the run."""
    san = str(tmp_path / "polygon_host_san")
    r = subprocess.run(["g++", "-O1", "-g", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all"] + FLAGS + ["-o", san, HARNESS],
                       capture_output=True, text=True)
    if r.returncode != 0 and ("asan" in r.stderr or "ubsan" in r.stderr or "sanitize" in r.stderr):
        pytest.skip("g++ here lacks the sanitizer runtimes: " + r.stderr.strip().splitlines()[-1])
    assert r.returncode == 0, r.stderr
    names = list(pl.CASES)
    got = run_host(san, tmp_path, names)
    for name in names:
        assert got[name].tobytes() == pl.literal(name).tobytes(), name


def test_host_core_refuses_what_the_library_refuses(exe, tmp_path):
    src, dst = str(tmp_path / "in"), str(tmp_path / "out")
    for ring, y_offset in (([], 0), ([[3, 2 ** 24 - 5]], 5), ([[-2 ** 24, 0]], 0)):
        with open(src, "wb") as f:
            f.write(np.array([1, 4, 4, 1], np.int32).tobytes())
            f.write(np.array([y_offset, 0], np.int64).tobytes())
            f.write(np.array([1, len(ring)], np.int32).tobytes())
            f.write(np.array(ring, np.int32).tobytes())
        assert subprocess.run([exe, src, dst]).returncode == 7


def test_python_argument_errors():
    from tmlibrary_amd import image
    from tmlibrary_amd.image import ContourPolygon
    from tmlibrary_amd.workflow.jterator.handles import SegmentedObjects

    ring = pl.rectangle(1, 1, 3, 3)
    assert image.polygon_ring(ring).dtype == np.int32
    assert np.array_equal(image.polygon_ring(ContourPolygon(ring, [ring])), ring)
    assert np.array_equal(image.polygon_ring(ring.astype(np.int64)), ring)

    class Shapely(object):  # what shapely's Polygon offers the reference
        class exterior(object):
            coords = [(1.9, -1.9), (3.2, -1.0), (3.0, -3.7)]

    assert image.polygon_ring(Shapely()).tolist() == [[1, -1], [3, -1], [3, -3]]
    with pytest.raises(ValueError):
        image.polygon_ring(np.zeros((0, 2), np.int32))
    with pytest.raises(ValueError):
        image.polygon_ring(ContourPolygon(np.zeros((0, 2), np.int32)))
    with pytest.raises(ValueError):
        image.polygon_ring(np.zeros((3, 3), np.int32))
    with pytest.raises(ValueError):
        image.polygon_ring(np.array([[2 ** 40, 0]], np.int64))
    with pytest.raises(TypeError):
        image.polygon_ring(np.zeros((3, 2), np.float64))
    # refused before anything is sent to a device
    with pytest.raises(ValueError):
        image.create_from_polygons([(1, np.zeros((0, 2), np.int32))], 0, 0, (4, 4))
    with pytest.raises(ValueError):
        image.create_from_polygons([(2 ** 31, ring)], 0, 0, (4, 4))
    with pytest.raises(ValueError):
        image.label_planes_from_polygons([[(1, ring)]], 0, 0, (0, 4))
    assert image.label_planes_from_polygons([], 0, 0, (3, 4)).shape == (0, 3, 4)
    assert not hasattr(image.SegmentationImage, "create_from_polygons")
    obj = SegmentedObjects("cells", "cells")
    with pytest.raises(ValueError):
        obj.add_polygons([], 0, 0, (4, 4))
    with pytest.raises(ValueError):
        obj.add_polygons([[[(1, ring)]], [[(1, ring)], []]], 0, 0, (4, 4))


def test_library_refuses_by_name_without_a_device():
    """The refusals the host form decides before it touches a device."""
    from tmlibrary_amd import hip

    lib = hip.load_library()
    pts = np.ascontiguousarray(pl.rectangle(1, 1, 3, 3))
    first = np.array([0, len(pts)], np.int64)
    plane, label = np.zeros(1, np.int32), np.ones(1, np.int32)
    out = np.full((1, 4, 4), -7, np.int32)

    def call(points=pts, first=first, plane=plane, label=label, n=1, n_planes=1, out=out,
             h=4, w=4):
        return lib.tmh_polygon_fill(hip.ptr(points), hip.ptr(first), hip.ptr(plane), hip.ptr(label),
                                    n, n_planes, h, w, 0, 0, hip.ptr(out))

    def refused(word, **kw):
        assert call(**kw) == hip.TMH_EINVAL
        assert word in lib.tmh_last_error().decode(), lib.tmh_last_error()
        assert (out == -7).all()

    refused("65,535", n_planes=65536)
    refused("geometry", h=0)
    refused("geometry", n=-1)
    refused("empty ring", first=np.array([0, 0], np.int64))
    refused("monotone", first=np.array([5, 0], np.int64))
    refused("monotone", first=np.array([-1, 4], np.int64))
    refused("out of range", n_planes=0)
    refused("overlaps", points=out.reshape(-1, 2)[:5])
    refused("overlaps", label=out.reshape(-1)[3:4])
    lib.tmh_polygon_fill.argtypes = None  # NULL pointers
    assert lib.tmh_polygon_fill(None, None, None, None, C.c_int64(1), C.c_int64(1), 4, 4,
                                C.c_int64(0), C.c_int64(0), hip.ptr(out)) == hip.TMH_EINVAL
    lib.tmh_polygon_fill.argtypes = hip.SIGNATURES["tmh_polygon_fill"][1]


def test_abi_exports():
    from tmlibrary_amd import hip

    text = open(os.path.join(REPO, "include", "tmhip.h")).read()
    lib = hip.load_library()
    for name in ("tmh_polygon_fill", "tmh_polygon_fill_device"):
        assert name in hip.SIGNATURES and name + "(" in text and hasattr(lib, name)
    assert "#define TMH_POLYGON_LDS_WORDS %d\n" % hip.POLYGON_LDS_WORDS in text
    assert lib.tmh_abi_version() == hip.ABI_VERSION
