"""GPU: jterator's site I/O -- the channel stack kernel, the object table
kernel, the handles and ``load_pipeline_inputs``.

Stack: the expected output is the existing device correction
(``Corrector.apply``) followed by numpy slicing with ``align_window(...,
crop=True)``, placed into [h, w, z, t]; the stack must equal it exactly.
Object table: every field equals the numpy literal (tests/objects_literal.py).
"""
import ctypes as C
import os

import numpy as np
import pytest

import intensity_cases as ic
import objects_literal as lit

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    from tmlibrary_amd import hip
    return hip.lib()


@pytest.fixture(scope="module")
def torch_():
    import torch
    return torch


# ---- channel stack ---------------------------------------------------------------

def stat_planes(H, W, channel=0):
    """A dim corner (small std: a large gain) so that bright pixels there pass
    the f32 bound and take the f64 refinement, as in real statistics."""
    yy, xx = np.mgrid[0:H, 0:W]
    mean = 2.45 + 0.1 * channel + 0.15 * np.exp(-((yy - H / 2.0) ** 2 + (xx - W / 2.0) ** 2)
                                                / (0.3 * H * W))
    std = 0.06 + 0.25 * (xx / float(W)) + 0.02 * channel
    return mean, std


def pixels(n, H, W, seed):
    rng = np.random.RandomState(seed)
    a = rng.randint(90, 1400, (n, H, W)).astype(np.uint16)
    a[rng.rand(n, H, W) < 0.01] = 0
    a[rng.rand(n, H, W) < 0.01] = 65535
    a[rng.rand(n, H, W) < 0.02] = 5000  # beyond the LDS log table
    return a


def windows_for(shape, residues, shifts):
    """One crop=True window per (y, x) shift under shared residues."""
    from tmlibrary_amd import hip
    from tmlibrary_amd.image import align_window
    top, bottom, left, right = residues
    out = np.zeros(len(shifts), dtype=hip.WINDOW_DTYPE)
    extent = None
    for i, (y, x) in enumerate(shifts):
        w, e = align_window(shape, y, x, bottom, top, right, left, crop=True)
        out[i] = w
        assert extent in (None, tuple(e))
        extent = tuple(e)
    return out, extent


def expected_stack(corrected, site, slot, win, n_sites, Z, T, extent):
    h, w = extent
    out = np.zeros((n_sites, h, w, Z, T), np.uint16)
    for p in range(len(site)):
        r0, c0 = int(win[p]["src_r0"]), int(win[p]["src_c0"])
        z, t = divmod(int(slot[p]), T)
        out[site[p], :, :, z, t] = corrected[p, r0:r0 + h, c0:c0 + w]
    return out.reshape(n_sites, h, w, Z * T)


_correctors = {}


def corrector(shape, log=True):
    from tmlibrary_amd.image import Corrector
    key = (tuple(shape), log)
    if key not in _correctors:
        mean, std = stat_planes(*shape)
        if not log:
            mean, std = mean * 200.0, std * 90.0
        _correctors[key] = Corrector(mean, std, log_transform=log)
    return _correctors[key]


#: shape, residues (top, bottom, left, right), per site shifts, (Z, T), log
STACK_CASES = [
    ((40, 56), (0, 0, 0, 0), [(0, 0)], (1, 1), True),             # whole image: the wide form
    ((40, 56), (2, 2, 5, 3), [(0, 0)], (1, 1), True),             # wide form, odd src_c0 = 5
    ((40, 56), (2, 2, 5, 3), [(2, -3)], (1, 1), False),           # wide form, even src_c0 = 8
    ((40, 56), (2, 2, 5, 3), [(-2, 5)], (2, 3), True),            # six slots, src_c0 = 0
    ((40, 56), (2, 2, 5, 3), [(1, 2)], (1, 4), True),             # four slots: 8-byte stores
    ((40, 56), (1, 3, 2, 2), [(1, -2)], (2, 1), False),           # two slots: 4-byte stores
    ((37, 57), (1, 2, 3, 2), [(0, 0)], (1, 1), True),             # odd width, odd src_c0 = 3
    ((37, 57), (1, 2, 3, 2), [(-2, 1)], (1, 1), True),            # odd width, even src_c0 = 2
    ((37, 57), (1, 2, 3, 2), [(1, 3), (0, -2)], (1, 3), False),   # odd width, three slots
    ((40, 56), (3, 1, 4, 4), [(3, 4), (-1, -4), (0, 0)], (1, 1), True),   # 3 sites, 3 origins
    ((40, 56), (3, 1, 4, 4), [(3, 4), (-1, -4), (0, 1)], (2, 2), True),
]


@pytest.mark.parametrize("shape,residues,shifts,zt,log", STACK_CASES)
def test_stack_equals_correct_then_crop(L, shape, residues, shifts, zt, log):
    from tmlibrary_amd.image import correct_stack
    Z, T = zt
    n_sites = len(shifts)
    site = np.repeat(np.arange(n_sites), Z * T).astype(np.int32)
    slot = np.tile(np.arange(Z * T), n_sites).astype(np.int32)
    perm = np.random.RandomState(3).permutation(site.size)  # planes in no particular order
    site, slot = site[perm], slot[perm]
    win_site, extent = windows_for(shape, residues, shifts)
    win = win_site[site]
    planes = pixels(site.size, shape[0], shape[1], seed=11)
    corr = corrector(shape, log)
    want = expected_stack(corr.apply(planes), site, slot, win, n_sites, Z, T, extent)
    got = correct_stack(corr, planes, site, slot, win, n_sites, Z * T, extent)
    assert got.shape == want.shape
    assert np.array_equal(got, want)
    # not corrected: a plain crop
    raw = correct_stack(None, planes, site, slot, win, n_sites, Z * T, extent)
    assert np.array_equal(raw, expected_stack(planes, site, slot, win, n_sites, Z, T, extent))


@pytest.mark.parametrize("zt", [(1, 1), (2, 3)])
def test_stack_unmapped_slot_is_zeroed(L, torch_, zt):
    """One (site, slot) without a plane is 0 in an output pre-filled with 0xFFFF."""
    Z, T = zt
    shape, n_sites = (40, 56), 2
    win_site, extent = windows_for(shape, (2, 2, 5, 3), [(1, 1), (-1, 0)])
    pairs = [(s, k) for s in range(n_sites) for k in range(Z * T)][:-1]  # the last one is dropped
    site = np.array([p[0] for p in pairs], np.int32)
    slot = np.array([p[1] for p in pairs], np.int32)
    win = np.ascontiguousarray(win_site[site])
    planes = pixels(len(pairs), shape[0], shape[1], seed=12)
    corr = corrector(shape, True)
    want = expected_stack(corr.apply(planes), site, slot, win, n_sites, Z, T, extent)
    assert not want[n_sites - 1, :, :, Z * T - 1].any()
    d_in = torch_.from_numpy(planes.view(np.int16)).cuda()
    d_out = torch_.full((n_sites, extent[0], extent[1], Z * T), -1, dtype=torch_.int16,
                        device="cuda")
    torch_.cuda.synchronize()
    from tmlibrary_amd import hip
    hip.check(L.tmh_correct_stack_u16_device(
        corr._h, C.c_void_p(d_in.data_ptr()), C.c_void_p(d_out.data_ptr()), len(pairs), shape[0],
        shape[1], hip.ptr(site), hip.ptr(slot), hip.ptr(win), n_sites, Z * T, extent[0], extent[1],
        None))
    got = d_out.cpu().numpy().view(np.uint16)
    assert np.array_equal(got, want)


def test_stack_rejects_bad_arguments(L):
    from tmlibrary_amd import hip
    from tmlibrary_amd.image import correct_stack
    shape = (40, 56)
    win, extent = windows_for(shape, (2, 2, 5, 3), [(0, 0), (1, 1)])
    planes = pixels(2, 40, 56, seed=13)
    corr = corrector(shape, True)
    site, slot = np.array([0, 0], np.int32), np.array([0, 1], np.int32)
    with pytest.raises(ValueError, match="two planes map to one"):
        correct_stack(corr, planes, site, np.array([1, 1], np.int32), win, 1, 2, extent)
    bad = win.copy()
    bad[1]["rows"] -= 1
    with pytest.raises(ValueError, match="could not broadcast"):
        correct_stack(corr, planes, site, slot, bad, 1, 2, extent)
    with pytest.raises(ValueError, match="slot index out of range"):
        correct_stack(corr, planes, site, np.array([0, 2], np.int32), win, 1, 2, extent)
    with pytest.raises(ValueError, match="site index out of range"):
        correct_stack(corr, planes, np.array([0, 1], np.int32), slot, win, 1, 2, extent)
    out = np.zeros((1, extent[0], extent[1], 2), np.uint16)
    rc = L.tmh_correct_stack_u16(corr._h, hip.ptr(planes), hip.ptr(out), 2, 40, 56, hip.ptr(site),
                                 hip.ptr(np.array([1, 1], np.int32)), hip.ptr(win), 1, 2,
                                 extent[0], extent[1])
    assert rc == hip.TMH_EINVAL


def test_stack_full_size_site(L):
    """One 2160 x 2560 site, slots = 1: the wide form at production size."""
    from tmlibrary_amd.image import correct_stack
    shape = (2160, 2560)
    win, extent = windows_for(shape, (7, 9, 11, 5), [(3, -2)])
    assert extent == (2144, 2544) and int(win[0]["src_c0"]) == 13
    planes = pixels(1, shape[0], shape[1], seed=14)
    corr = corrector(shape, True)
    zero = np.zeros(1, np.int32)
    want = expected_stack(corr.apply(planes), zero, zero, win, 1, 1, 1, extent)
    got = correct_stack(corr, planes, zero, zero, win, 1, 1, extent)
    assert np.array_equal(got, want)


# ---- object table ----------------------------------------------------------------

def cells(h, w, n, seed):
    """About n random cells: nearest-seed labels 1..n, with background gaps."""
    rng = np.random.RandomState(seed)
    sy, sx = rng.randint(0, h, n), rng.randint(0, w, n)
    plane = np.zeros((h, w), np.int32)
    best = np.full((h, w), np.inf)
    yy, xx = np.mgrid[0:h, 0:w]
    for k in range(n):  # a window around each seed is enough at this density
        r = 40
        y0, y1, x0, x1 = max(0, sy[k] - r), min(h, sy[k] + r), max(0, sx[k] - r), min(w, sx[k] + r)
        d = (yy[y0:y1, x0:x1] - sy[k]) ** 2 + (xx[y0:y1, x0:x1] - sx[k]) ** 2
        sub = best[y0:y1, x0:x1]
        m = d < sub
        sub[m] = d[m]
        plane[y0:y1, x0:x1][m] = k + 1
    plane[best > 60] = 0
    return plane


def check_tables(planes, max_label=None):
    from tmlibrary_amd.image import object_tables
    planes = np.ascontiguousarray(planes, dtype=np.int32)
    got = object_tables(planes)
    top = max(int(planes.max()), 0) if max_label is None else max_label
    assert got.shape == (planes.shape[0], top + 1)
    for p in range(planes.shape[0]):
        want = lit.object_rows(planes[p], top)
        for name in lit.ROW_DTYPE.names:
            assert np.array_equal(got[p][name], want[name]), (p, name)
    return got


def runs_plane():
    """64 x 200: runs crossing lane 63 / 64 and row ends, and the same label at
    the end of one row and the start of the next."""
    plane = np.zeros((64, 200), np.int32)
    plane[0, 60:70] = 1            # crosses lane 63 | 64
    plane[1, 120:135] = 2          # crosses lane 127 | 128
    plane[2, 190:200] = 3          # ends a row ...
    plane[3, 0:5] = 3              # ... and starts the next: two runs, not one
    plane[4, 63] = 4
    plane[4, 64] = 5
    plane[5, :] = 6                # a whole row
    plane[10:20, 63:65] = 7
    plane[30, 199] = 8
    plane[31, 0] = 8
    plane[63, 100:192] = 9         # last row, crossing two lane boundaries
    return plane


def test_objects_small_planes(L):
    check_tables(np.zeros((1, 9, 11), np.int32))
    check_tables(np.full((1, 5, 7), 4, np.int32))
    check_tables((np.arange(130, dtype=np.int32) // 7 % 5).reshape(1, 1, 130))
    check_tables((np.arange(130, dtype=np.int32) // 3 % 4).reshape(1, 130, 1))
    yy, xx = np.mgrid[0:33, 0:70]
    check_tables(((yy + xx) % 2 + 1).astype(np.int32)[None])  # runs of length 1
    got = check_tables(runs_plane()[None])
    assert got[0][3]["n"] == 15 and got[0][3]["sum_x"] == sum(range(190, 200)) + sum(range(5))


def test_objects_sparse_labels(L):
    plane = np.zeros((20, 30), np.int32)
    plane[2:5, 3:9] = 3
    plane[10:12, 20:30] = 70000
    got = check_tables(plane[None])
    assert got.shape == (1, 70001)
    absent = np.ones(70001, bool)
    absent[[0, 3, 70000]] = False
    assert not got[0][absent].view(np.uint8).any()  # rows of absent labels all zero


def test_objects_random_cells(L):
    plane = cells(300, 517, 2000, seed=21)
    plane[0, :] = 0
    plane[-1, :] = 0
    plane[:, 0] = 0
    plane[:, -1] = 0
    top = int(plane.max())
    plane[0, 100:103] = top + 1      # one label on each edge only
    plane[-1, 200:204] = top + 2
    plane[50:53, 0] = top + 3
    plane[80:82, -1] = top + 4
    got = check_tables(plane[None])
    assert len(lit.labels(plane)) > 1000
    assert got[0]["border"][top + 1:top + 5].tolist() == [1, 1, 1, 1]
    inner = [k for k in lit.labels(plane) if k <= top]
    assert not got[0]["border"][inner].any()


def test_objects_five_planes_one_call(L):
    planes = np.zeros((5, 45, 70), np.int32)
    for p in range(5):
        planes[p] = cells(45, 70, 6 + 3 * p, seed=30 + p) * (p + 1)  # different label sets
    planes[2] = 0
    check_tables(planes)


def test_objects_full_size_single_label(L):
    plane = np.full((1, 2160, 2560), 1, np.int32)
    got = check_tables(plane)
    assert got[0][1]["sum_x"] == 2160 * (2560 * 2559 // 2) > 2 ** 32


# The table kernel's memory route (objects_kernels.hip k_object_table: a label
# that finds no LDS entry within TMH_OBJECT_PROBE probes goes through
# object_add_global to its row in memory).  Which labels of a full tile get the
# entries depends on the order the waves run in; that more labels than entries
# take memory does not.

def tile_label_counts(plane):
    """{(tile row, tile column): distinct labels} of k_object_table's 16 x 512 tiles."""
    return {(ty, tx): len(np.unique(plane[16 * ty:16 * ty + 16, 512 * tx:512 * tx + 512]))
            for ty in range(-(-plane.shape[0] // 16)) for tx in range(-(-plane.shape[1] // 512))}


def one_label_per_pixel():
    """(1, 16, 512): one tile, the labels 1..8192 in a random order."""
    return (np.random.RandomState(61).permutation(8192) + 1).astype(np.int32).reshape(1, 16, 512)


def test_objects_one_label_per_pixel(L):
    """k_object_table's else branch (object_add_global from the pixel loop): a
    single tile with 8,192 labels and 512 LDS entries, so at least 7,680 labels
    are added to rows still holding k_object_init's INT_MAX / -1 bounds; every
    field of every row against the literal, the border flags included (1,052
    labels lie on the plane's edge)."""
    from tmlibrary_amd import hip
    planes = one_label_per_pixel()
    assert tile_label_counts(planes[0]) == {(0, 0): 8192} and 8192 > hip.OBJECT_SLOTS
    got = check_tables(planes)
    assert int(got[0]["border"].sum()) == 2 * 512 + 2 * 14
    assert np.array_equal(got[0]["n"][1:], np.ones(8192, np.int64))


def test_objects_mixed_routes_across_tiles(L):
    """k_object_table, both routes into the same rows: three planes of 33 x
    1030 (3 x 3 ragged tiles each) with a label in every pixel, runs of length
    one, up to 3,000 labels.  The four 16 x 512 tiles of each plane hold more
    labels than the LDS table has entries, so each sends its surplus through
    object_add_global; the narrow and the one-row tiles hold few enough to
    keep theirs in LDS (at most TMH_OBJECT_PROBE labels: certainly), and their
    labels recur in the full tiles, so rows take flushed LDS entries and direct
    adds alike.  Planes 1 and 2 have label sets of their own and write at row
    offset plane * (max_label + 1); labels sit on all four edges."""
    from tmlibrary_amd import hip
    H, W = 33, 1030
    idx = np.arange(H * W, dtype=np.int64).reshape(H, W)
    rng = np.random.RandomState(62)
    planes = np.stack([idx * 7919 % 3000 + 1,
                       idx * 7919 % 2500 + 401,
                       rng.randint(1001, 3001, (H, W))]).astype(np.int32)
    assert planes.max() == 3000 and planes.min() >= 1
    for p in range(3):
        counts = tile_label_counts(planes[p])
        assert len(counts) == 9
        full = [counts[(ty, tx)] for ty in (0, 1) for tx in (0, 1)]
        assert min(full) > hip.OBJECT_SLOTS, full
        assert counts[(2, 2)] <= hip.OBJECT_PROBE  # the 1 x 6 corner: LDS for certain
        corner = set(planes[p][32:, 1024:].ravel().tolist())
        assert corner <= set(planes[p][:32, :1024].ravel().tolist())
    assert len({frozenset(np.unique(pl).tolist()) for pl in planes}) == 3
    got = check_tables(planes)
    for p in range(3):
        edge = np.unique(np.concatenate([planes[p][0], planes[p][-1], planes[p][:, 0],
                                         planes[p][:, -1]]))
        assert got[p]["border"][edge].all() and int(got[p]["border"].sum()) == len(edge)


def test_objects_probe_limit_in_a_nearly_empty_table(L):
    """k_object_table's probe loop giving up (t == kObjProbe) with the table
    almost empty: TMH_OBJECT_PROBE + 8 labels hash to entry 7 of one tile, the
    first to arrive fill entries 7 .. 7 + TMH_OBJECT_PROBE - 1, and the other 8
    find no entry although some 480 are free -- they go to memory, two runs
    each (2 x 3 blocks: the second add meets the first's bounds, not the
    initial ones)."""
    from tmlibrary_amd import hip
    labels = ic.same_bucket_labels(7, hip.OBJECT_PROBE + 8, hip.OBJECT_SLOTS)
    if hip.OBJECT_SLOTS == 512:
        assert labels[:5] == [267, 644, 1254, 1864, 2241]
    plane = np.zeros((16, 512), np.int32)
    for k, label in enumerate(labels):
        r, c = 1 + 4 * (k // 12), 5 + 40 * (k % 12)
        plane[r:r + 2, c:c + 3] = label
    assert tile_label_counts(plane) == {(0, 0): len(labels) + 1}
    got = check_tables(plane[None])
    assert got[0]["n"][labels].tolist() == [6] * len(labels)
    assert int(np.count_nonzero(got[0]["n"])) == len(labels) + 1


def test_objects_one_label_per_pixel_outlines(L):
    """The outlines start from the table rows the memory route wrote
    (contour_kernels.hip reads each label's bbox from them): 8,192 one-pixel
    objects, each the second fallback (no opening, one point), against the
    plain-loop literal."""
    import contours_literal as cl
    from test_gpu_contours import assert_equal_literal
    from tmlibrary_amd.image import object_contours
    planes = one_label_per_pixel()
    rows, objects, contours, points = object_contours(planes)
    want = lit.object_rows(planes[0], 8192)
    for name in lit.ROW_DTYPE.names:
        assert np.array_equal(rows[0][name], want[name]), name
    assert_equal_literal((objects, contours, points), cl.object_contours(planes))


@pytest.mark.parametrize("bad,message", [(-1, "negative label"), (8, "above max_label")])
def test_objects_reject_labels_out_of_range(L, torch_, bad, message):
    from tmlibrary_amd import hip
    plane = (np.arange(40 * 50, dtype=np.int32) % 8).reshape(40, 50)
    plane[17, 23] = bad
    d_plane = torch_.from_numpy(plane).cuda()
    n_rows, guard = 8, 64
    d_rows = torch_.full((guard + n_rows * 48 + guard,), 0x5A, dtype=torch_.uint8, device="cuda")
    torch_.cuda.synchronize()
    rc = L.tmh_object_table_device(C.c_void_p(d_plane.data_ptr()), 1, 40, 50, 7,
                                   C.c_void_p(d_rows.data_ptr() + guard), None)
    assert rc == hip.TMH_EINVAL and message in L.tmh_last_error().decode()
    assert L.tmh_synchronize(None) == 0
    assert bool((d_rows == 0x5A).all())  # rows and guard regions untouched
    if bad < 0:
        from tmlibrary_amd.image import object_tables
        with pytest.raises(ValueError, match="negative label"):
            object_tables(plane[None])


def test_label_max_device(L, torch_):
    planes = np.zeros((3, 33, 47), np.int32)
    planes[0, 5, 5] = 9
    planes[1, 32, 46] = 123456
    planes[1, 0, 0] = -7
    planes[2] = 4
    d = torch_.from_numpy(planes).cuda()
    mx = torch_.zeros(3, dtype=torch_.int32, device="cuda")
    mn = torch_.zeros(3, dtype=torch_.int32, device="cuda")
    torch_.cuda.synchronize()
    assert L.tmh_label_max_device(C.c_void_p(d.data_ptr()), 3, 33, 47, C.c_void_p(mx.data_ptr()),
                                  C.c_void_p(mn.data_ptr()), None) == 0
    assert L.tmh_synchronize(None) == 0
    assert mx.cpu().tolist() == [9, 123456, 4] and mn.cpu().tolist() == [0, -7, 4]


# ---- handles ---------------------------------------------------------------------

def handle_value():
    value = np.zeros((45, 70, 2, 2), np.int32)
    base = cells(45, 70, 9, seed=40)
    yy, xx = np.mgrid[0:45, 0:70]
    for z in range(2):
        for t in range(2):
            # every label in every plane; whole discs have integer centroids, so
            # each plane loses another set of pixels, which breaks the symmetry
            plane = base.copy()
            plane[(yy * (7 + z) + xx * (3 + 2 * t)) % 11 == 0] = 0
            value[:, :, z, t] = plane
    return value


@pytest.mark.parametrize("offsets", [(-17, 9), (23, -4)])
def test_segmented_objects_equal_literal(L, offsets):
    from tmlibrary_amd.workflow.jterator.handles import SegmentedObjects
    value = handle_value()
    obj = SegmentedObjects("cells", "cells")
    obj.value = value
    assert obj.labels == lit.labels(value) and len(obj.labels) >= 5
    assert obj.is_border == lit.is_border(value)
    # the condition on the inputs: no centroid within 1e-9 of an integer
    for c in lit.centroids_before_int(value, *offsets).values():
        c = c[obj.labels]
        assert np.all(np.abs(c - np.round(c)) > 1e-9)
    assert list(obj.iter_points(*offsets)) == list(lit.iter_points(value, *offsets))


def test_iter_points_absent_label_raises(L):
    from tmlibrary_amd.workflow.jterator.handles import SegmentedObjects
    value = handle_value()
    value[:, :, 1, 0][value[:, :, 1, 0] == 2] = 0  # label 2 is absent from one plane
    obj = SegmentedObjects("cells", "cells")
    obj.value = value
    assert 2 in obj.labels
    with pytest.raises(ValueError):
        list(lit.iter_points(value, 0, 0))
    with pytest.raises(ValueError):
        list(obj.iter_points(0, 0))


def test_segmentation_image_bboxes(L):
    from tmlibrary_amd.image import SegmentationImage
    plane = cells(45, 70, 9, seed=41)
    img = SegmentationImage(plane)
    assert np.array_equal(img.bboxes(), lit.bbox(plane))
    assert np.array_equal(img.object_table()["n"], lit.object_rows(plane)["n"])


# ---- load_pipeline_inputs --------------------------------------------------------

def _store(tmp_path):
    """2 sites x 2 channels (channel 0 in cycle 0 corrected, channel 1 in cycle
    1 not) x 2 z-planes of 96 x 128 files, written with the repository's writer."""
    from tmlibrary_amd.models.file import ExperimentStore, write_channel_image, write_illumstats
    os.makedirs(str(tmp_path / "channel_image_files"))
    info, images = {}, {}
    fid = 0
    for site in (0, 1):
        for channel in (0, 1):
            for z in (0, 1):
                info[fid] = (channel, site, channel, 0, z)
                images[fid] = pixels(1, 96, 128, seed=50 + fid)[0]
                fid += 1
    store = ExperimentStore(str(tmp_path), file_info=info)
    for f, img in images.items():
        write_channel_image(store.channel_image_file(f).location, img, gzip_level=4)
    mean, std = stat_planes(96, 128)
    write_illumstats(store.illumstats_file(0).location, mean, std, {50.0: 300})
    store.site_shifts = {(0, 0): (0, 0), (0, 1): (2, -3), (1, 0): (0, 0), (1, 1): (-1, 4)}
    res = dict(top=2, bottom=1, left=4, right=3)
    store.site_residues = {0: res, 1: res}
    store.channel_names = {"dapi": 0, "gfp": 1}
    return store, images


@pytest.mark.parametrize("decode", ["auto", "host"])
def test_load_pipeline_inputs(L, tmp_path, decode):
    from tmlibrary_amd.models.file import h5lib
    from tmlibrary_amd.workflow.jterator import api as japi
    h5lib()
    store, images = _store(tmp_path)
    pipe = japi.ImageAnalysisPipeline(1, store=store, decode=decode)
    channels = [("dapi", True), ("gfp", False)]
    stores = pipe.load_pipeline_inputs([0, 1], channels)
    assert pipe.last_path == ("gpu" if decode == "auto" else "host")
    corr = store.illumstats_file(0).get().corrector()  # the existing device path
    res = store.site_residues[0]
    for k, site in enumerate((0, 1)):
        st = stores[k]
        assert sorted(st) == ["channels", "current_figure", "objects", "pipe", "site_id"]
        assert st["site_id"] == site and sorted(st["pipe"]) == ["dapi", "gfp"]
        for name, correct in channels:
            ch = store.channel_names[name]
            image_array = np.zeros((96 - 3, 128 - 7, 2, 1), np.uint16)
            for fid, (c, s, cycle, tpoint, zplane) in store.file_info.items():
                if (c, s) != (ch, site):
                    continue
                img = corr.apply(images[fid]) if correct else images[fid]
                y, x = store.site_shifts[(s, cycle)]
                rs, re_ = res["top"] - y, res["bottom"] + y
                cs, ce = res["left"] - x, res["right"] + x
                img = img[rs:(96 if re_ == 0 else -re_), cs:(128 if ce == 0 else -ce)]
                image_array[:, :, zplane, tpoint] = img
            want = np.squeeze(image_array)
            assert st["pipe"][name].shape == want.shape == (93, 121, 2)
            assert np.array_equal(st["pipe"][name], want), (site, name)
    one = pipe.load_pipeline_input(1, channels)
    for name, _ in channels:
        assert np.array_equal(one["pipe"][name], stores[1]["pipe"][name])
    corr.close()


def test_missing_illumstats_raises(L, tmp_path):
    from tmlibrary_amd.workflow.jterator import api as japi
    store, _ = _store(tmp_path)
    pipe = japi.ImageAnalysisPipeline(1, store=store)
    with pytest.raises(japi.PipelineDescriptionError,
                       match='No illumination statistics file found for channel "gfp"'):
        pipe.load_pipeline_input(0, [("gfp", True)])
