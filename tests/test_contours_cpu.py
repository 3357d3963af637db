"""CPU: the outline rules and the kernel's core.

tests/contours_literal.py restates the opening and Suzuki and Abe's border
following in plain loops; tmlibrary_amd/csrc/contour_core.h is the code
the contour kernels run, compiled here with g++ through tests/contour_host.cpp.
Both go through the same cases: two hand-traced anchors, properties that hold
for any correct border follower (so no restatement is trusted on its own), the
opening against scipy across word boundaries, and the GPU tests' planes.
"""
import os
import subprocess

import numpy as np
import pytest
from scipy import ndimage as ndi

import contour_cases as cc
import contours_literal as cl
from util import REPO

HARNESS = os.path.join(REPO, "tests", "contour_host.cpp")
FLAGS = ["-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas"]
EIGHT = np.ones((3, 3), bool)


def run_host(exe, tmp_path, masks):
    """[(mask, open)] -> [(mask after the opening, borders as find_contours gives them)]."""
    src, dst = str(tmp_path / "in"), str(tmp_path / "out")
    with open(src, "wb") as f:
        f.write(np.array([len(masks)], np.int32).tobytes())
        for m, do_open in masks:
            f.write(np.array([m.shape[0], m.shape[1], do_open], np.int32).tobytes())
            f.write(np.ascontiguousarray(m, dtype=np.uint8).tobytes())
    subprocess.run([exe, src, dst], check=True)
    raw, at, out = open(dst, "rb").read(), 0, []
    for m, _ in masks:
        h, w = m.shape
        opened = np.frombuffer(raw, np.uint8, h * w, at).reshape(h, w).astype(bool)
        at += h * w
        n = int(np.frombuffer(raw, np.int32, 1, at)[0])
        at += 4
        borders = []
        for _ in range(n):
            is_hole, parent, k = (int(v) for v in np.frombuffer(raw, np.int32, 3, at))
            at += 12
            borders.append((np.frombuffer(raw, np.int32, 2 * k, at).reshape(k, 2), is_hole, parent))
            at += 8 * k
        out.append((opened, borders))
    assert at == len(raw)
    return out


def literal_run(masks):
    out = []
    for m, do_open in masks:
        m = cl.open_cross(m) if do_open else np.asarray(m, bool)
        out.append((m, cl.find_contours(m)))
    return out


def same_borders(a, b):
    return len(a) == len(b) and all(
        x[1] == y[1] and x[2] == y[2] and x[0].dtype == y[0].dtype == np.int32
        and x[0].tobytes() == y[0].tobytes() for x, y in zip(a, b))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("contour") / "contour_host")
    subprocess.run(["g++", "-O2"] + FLAGS + ["-o", out, HARNESS], check=True, capture_output=True)
    return out


@pytest.fixture(scope="module")
def random_masks():
    """300 seeded masks up to 13 x 13 (padded: up to 15 x 15) at densities 0.3
    to 0.9, every second one opened first."""
    rng = np.random.default_rng(21)
    out = []
    for i in range(300):
        h, w = (int(v) for v in rng.integers(1, 14, 2))
        m = rng.random((h, w)) < rng.uniform(0.3, 0.9)
        out.append((np.pad(m, 1), i % 2))
    return out


@pytest.fixture(scope="module")
def plane_masks():
    """the mask of every object of the GPU tests' planes"""
    out = []
    for name, _ in cc.SMALL_PLANES:
        out += cc.masks_of(cc.literal(name)[0])
    for args in (("switch", 16384), ("switch", 4096), ("switch", 1024), ("single",), ("voronoi",)):
        out += cc.masks_of(cc.literal(*args)[0])
    return out


def anchors():
    a = np.zeros((5, 7), bool)
    a[1:4, 2:5] = True
    b = a.copy()
    b[2, 3] = False
    return a, b


ANCHOR_OUTER = [(2, 1), (2, 2), (2, 3), (3, 3), (4, 3), (4, 2), (4, 1), (3, 1)]
ANCHOR_HOLE = [(2, 2), (3, 1), (4, 2), (3, 3)]


def check_anchors(results):
    (_, solid), (_, holed) = results
    assert len(solid) == 1 and solid[0][1:] == (0, -1)
    assert [tuple(p) for p in solid[0][0]] == ANCHOR_OUTER
    assert len(holed) == 2 and holed[0][1:] == (0, -1) and holed[1][1:] == (1, 0)
    assert [tuple(p) for p in holed[0][0]] == ANCHOR_OUTER
    assert [tuple(p) for p in holed[1][0]] == ANCHOR_HOLE


def check_properties(mask, borders):
    """What any correct 8-connected border follower gives for `mask`."""
    mask = np.asarray(mask, bool)
    comp, n_comp = ndi.label(mask, EIGHT)
    outers = [b for b in borders if not b[1]]
    holes = [b for b in borders if b[1]]
    assert len(outers) == n_comp
    _, n_bg = ndi.label(~mask)  # 4-connected background of the padded mask
    assert len(holes) == n_bg - 1
    # the union of all points: the 1-pixels with a zero 4-neighbour
    pad = np.pad(mask, 1)
    edge = mask & ~(pad[:-2, 1:-1] & pad[2:, 1:-1] & pad[1:-1, :-2] & pad[1:-1, 2:])
    seen = np.zeros_like(mask)
    for pts, _, _ in borders:
        assert pts.dtype == np.int32 and pts.ndim == 2 and pts.shape[1] == 2 and len(pts) > 0
        seen[pts[:, 1], pts[:, 0]] = True
        if len(pts) > 1:
            step = np.abs(pts - np.roll(pts, -1, axis=0))
            assert step.max() == 1 and (step.sum(axis=1) > 0).all()
    assert np.array_equal(seen, edge)
    for pts, _, parent in outers:
        x, y = pts[0]
        ys, xs = np.nonzero(comp == comp[y, x])
        assert (y, x) == (ys[0], xs[0])  # np.nonzero is in raster order
        assert parent == -1
    for pts, _, parent in holes:
        assert 0 <= parent < len(borders) and not borders[parent][1]
        a, b = pts[0], borders[parent][0][0]
        assert comp[a[1], a[0]] == comp[b[1], b[0]]


def test_literal_anchors():
    check_anchors(literal_run([(m, 0) for m in anchors()]))


def test_host_core_anchors(exe, tmp_path):
    check_anchors(run_host(exe, tmp_path, [(m, 0) for m in anchors()]))


def test_literal_properties(random_masks):
    results = literal_run(random_masks)
    assert len(results) == 300
    for mask, borders in results:
        check_properties(mask, borders)


def test_host_core_properties(exe, tmp_path, random_masks):
    results = run_host(exe, tmp_path, random_masks)
    assert len(results) == 300
    for mask, borders in results:
        check_properties(mask, borders)


def test_host_core_equals_literal(exe, tmp_path, random_masks, plane_masks):
    masks = [(m, 0) for m in anchors()] + random_masks + plane_masks
    got, want = run_host(exe, tmp_path, masks), literal_run(masks)
    assert len(got) == len(want) == len(masks)
    for i, ((gm, gb), (wm, wb)) in enumerate(zip(got, want)):
        assert np.array_equal(gm, wm), i
        assert same_borders(gb, wb), i


@pytest.mark.parametrize("width", [63, 64, 65, 130])
def test_opening_equals_scipy_across_words(exe, tmp_path, width):
    rng = np.random.default_rng(width)
    masks = []
    for density in (0.5, 0.8, 0.95):
        m = rng.random((9, width)) < density
        m[:, 60:68] |= rng.random((9, min(width, 68) - 60)) < 0.9  # busy at the word boundary
        masks.append((np.pad(m, 1), 1))
    for (m, _), (opened, _) in zip(masks, run_host(exe, tmp_path, masks)):
        assert m.shape[1] == width + 2
        want = ndi.binary_opening(m, ndi.generate_binary_structure(2, 1))
        assert np.array_equal(opened, want)
        assert want.sum() < m.sum()  # the opening did remove something


def test_case_list_under_sanitizers(tmp_path, random_masks, plane_masks):
    """The stand-alone harness built with -fsanitize=address,undefined: masks
    and marks are heap blocks of their exact size, so a neighbour read or a
    mark written outside a box ends the run."""
    san = str(tmp_path / "contour_host_san")
    r = subprocess.run(["g++", "-O1", "-g", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all"] + FLAGS + ["-o", san, HARNESS],
                       capture_output=True, text=True)
    if r.returncode != 0 and ("asan" in r.stderr or "ubsan" in r.stderr or "sanitize" in r.stderr):
        pytest.skip("g++ here lacks the sanitizer runtimes: " + r.stderr.strip().splitlines()[-1])
    assert r.returncode == 0, r.stderr
    masks = [(m, 0) for m in anchors()] + random_masks + plane_masks
    got = run_host(san, tmp_path, masks)
    assert len(got) == len(masks)
    for (gm, gb), (wm, wb) in zip(got[:40], literal_run(masks[:40])):
        assert np.array_equal(gm, wm) and same_borders(gb, wb)


def test_shell_and_holes_choice():
    """Rule 4 as the reference wrote it, over the cv2-shaped list."""
    from tmlibrary_amd.image import cv2_shaped, select_shell_and_holes

    _, holed = anchors()
    found = cl.find_contours(holed)
    contours, hierarchy = cv2_shaped([b[0] for b in found], [b[2] for b in found])
    want_c, want_h = cl.cv2_shaped(found)
    assert np.array_equal(hierarchy, want_h)
    assert all(np.array_equal(a, b) for a, b in zip(contours, want_c))
    assert [len(c) for c in contours] == [4, 8]  # reverse discovery order
    assert hierarchy[0].tolist() == [[-1, -1, -1, 1], [-1, -1, 0, -1]]
    shell, holes = select_shell_and_holes(contours, hierarchy)
    assert [tuple(p) for p in shell] == ANCHOR_OUTER
    assert len(holes) == 1 and [tuple(p) for p in holes[0]] == ANCHOR_HOLE


def test_polygon_without_shapely():
    from tmlibrary_amd.image import ContourPolygon
    from tmlibrary_amd.workflow.align.api import NotSupportedError

    poly = ContourPolygon(cl.square(3, 4), None)
    assert poly.shell.dtype == np.int32 and poly.shell.shape == (5, 2) and poly.holes == []
    try:
        import shapely  # noqa: F401
    except ImportError:
        with pytest.raises(NotSupportedError):
            poly.to_shapely()
    else:
        assert poly.to_shapely().exterior is not None
