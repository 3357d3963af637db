#!/usr/bin/env python3
"""Object outlines at full size on one MI355X.

Per content -- 16 label planes of 2160 x 2560 with about 2,000 and about
50,000 Voronoi cells (four distinct planes, each four times), and one plane of
two nested ring labels, whose boxes take the in-memory form:
  * ``tmh_object_contours_device`` writing its result: HIP-event time of count
    pass + scan + write pass per plane (``tmh_profile_read("contours")``), its
    ratio to the box's flat read of the plane (``tmh_box_probe_device`` mode
    3), and the object table alone (``"objects"``);
  * the host core -- tests/contour_host.cpp over contour_core.h, ``g++ -O2``,
    the same opening and border follower -- on sixteen processes, one plane's
    pre-cut masks each.  cv2 and mahotas are not installed here, so the host
    core stands in for the reference's per-object loop; it leaves out the
    loop's bounding-box cuts and its Python.
  * plane 0 of the device result checked against the host core's output.

    python tools/bench_contours.py [--out profiles/r16/bench_contours.json]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench_jterator import H, W, box_rates, voronoi  # noqa: E402
from bench_pyramid import kernel_ms  # noqa: E402
from tmlibrary_amd import hip  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROCESSES = 16


def nested_rings():
    p = np.zeros((H, W), np.int32)
    p[:, :] = 1
    p[200:H - 200, 200:W - 200] = 0
    p[300:H - 300, 300:W - 300] = 2
    p[500:H - 500, 500:W - 500] = 0
    return p


def plane_masks(plane):
    """[(label, padded mask before the opening, open flag)] as image.py:807-821 cuts them."""
    import scipy.ndimage as ndi
    boxes = ndi.find_objects(plane)
    plane0 = plane.copy()
    plane0[0, :] = plane0[-1, :] = 0
    plane0[:, 0] = plane0[:, -1] = 0
    out = []
    for label, sl in enumerate(boxes, start=1):
        if sl is None:
            continue
        mask = np.pad(plane0[sl] == label, 1)
        n = int(mask.sum())
        if n:
            out.append((label, mask, 1 if n > 1 else 0))
    return out


def write_cases(path, masks):
    with open(path, "wb") as f:
        f.write(np.array([len(masks)], np.int32).tobytes())
        for _, m, do_open in masks:
            f.write(np.array([m.shape[0], m.shape[1], do_open], np.int32).tobytes())
            f.write(np.ascontiguousarray(m, dtype=np.uint8).tobytes())


def read_borders(path, masks):
    """[(label, [(is_hole, parent, points)])] from the harness's output."""
    raw, at, out = open(path, "rb").read(), 0, []
    for label, m, _ in masks:
        at += m.size
        n = int(np.frombuffer(raw, np.int32, 1, at)[0])
        at += 4
        borders = []
        for _ in range(n):
            is_hole, parent, k = (int(v) for v in np.frombuffer(raw, np.int32, 3, at))
            at += 12
            borders.append((is_hole, parent, np.frombuffer(raw, np.int32, 2 * k, at).reshape(k, 2)))
            at += 8 * k
        out.append((label, borders))
    assert at == len(raw)
    return out


def host_core(exe, tmp, plane):
    masks = plane_masks(plane)
    src = os.path.join(tmp, "cases")
    write_cases(src, masks)
    t0 = time.perf_counter()
    procs = [subprocess.Popen([exe, src, os.path.join(tmp, "out%d" % i)]) for i in range(PROCESSES)]
    codes = [p.wait() for p in procs]
    dt = time.perf_counter() - t0
    assert not any(codes), codes
    stats = {"processes": PROCESSES, "planes": PROCESSES, "seconds": round(dt, 3),
             "ms_per_plane": round(dt / PROCESSES * 1e3, 2),
             "note": "contour_host (g++ -O2) stands in for cv2 + mahotas, which are not installed"}
    return stats, read_borders(os.path.join(tmp, "out0"), masks)


def same_as_host(objects, contours, points, want):
    for label, borders in want:
        o = objects[label]
        if o["n_contours"] != len(borders):
            return False
        table = contours[o["first_contour"]:o["first_contour"] + o["n_contours"]]
        for c, (is_hole, parent, pts) in zip(table, borders):
            got = points[c["point_offset"]:c["point_offset"] + c["n_points"]]
            if (c["is_hole"], c["parent"]) != (is_hole, parent) or not np.array_equal(got, pts):
                return False
    return int((objects["n_contours"] > 0).sum()) == sum(1 for _, b in want if b)


def bench_content(L, torch, exe, name, planes, warmup, reps, read_gbs):
    dev = torch.device("cuda", 0)
    n = planes.shape[0]
    d = torch.from_numpy(planes).to(dev)
    top = int(planes.max())
    n_rows = n * (top + 1)
    rows = torch.empty((n_rows * 48,), dtype=torch.uint8, device=dev)
    objs = torch.empty((n_rows * 64,), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    P = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    nc, npt = C.c_int64(0), C.c_int64(0)
    hip.check(L.tmh_profile_enable(0))
    hip.check(L.tmh_object_table_device(P(d), n, H, W, top, P(rows), None))
    hip.check(L.tmh_object_contours_device(P(d), n, H, W, top, P(rows), P(objs), None, 0, None, 0,
                                           C.byref(nc), C.byref(npt), None))
    con = torch.empty((max(nc.value, 1) * 32,), dtype=torch.uint8, device=dev)
    pts = torch.empty((max(npt.value, 1) * 2,), dtype=torch.int32, device=dev)

    def call():
        hip.check(L.tmh_object_table_device(P(d), n, H, W, top, P(rows), None))
        hip.check(L.tmh_object_contours_device(P(d), n, H, W, top, P(rows), P(objs), P(con),
                                               nc.value, P(pts), npt.value, C.byref(nc),
                                               C.byref(npt), None))
        hip.check(L.tmh_synchronize(None))

    for _ in range(warmup):
        call()
    walls = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        walls.append(time.perf_counter() - t0)
    hip.check(L.tmh_profile_enable(1))
    hip.check(L.tmh_profile_reset())
    for _ in range(reps):
        call()
    ms_c, _ = kernel_ms(L, "contours")
    ms_o, _ = kernel_ms(L, "objects")
    hip.check(L.tmh_profile_enable(0))
    objects = objs.cpu().numpy().view(hip.CONTOUR_OBJECT_DTYPE).reshape(n, top + 1)
    contours = con.cpu().numpy().view(hip.CONTOUR_DTYPE)[:nc.value]
    points = pts.cpu().numpy().reshape(-1, 2)[:npt.value]
    print("%s: device done, host core" % name, file=sys.stderr, flush=True)
    with tempfile.TemporaryDirectory() as tmp:
        host, want = host_core(exe, tmp, planes[0])
    per_plane = ms_c / (reps * n)
    flat = H * W * 4 / (read_gbs * 1e6)
    return {"content": name, "planes_per_call": n,
            "objects_per_plane": int((objects["n_interior"][0] > 0).sum()),
            "contours": int(nc.value), "points": int(npt.value),
            "contours_ms_per_plane": round(per_plane, 4),
            "flat_read_ms_per_plane": round(flat, 4),
            "x_flat_read": round(per_plane / flat, 1),
            "object_table_ms_per_plane": round(ms_o / (reps * n), 4),
            "call_wall_ms_per_plane": round(float(np.median(walls)) * 1e3 / n, 4),
            "equals_host_core_plane0": bool(same_as_host(objects[0], contours, points, want)),
            "host_core": host,
            "x_host_core": round(host["ms_per_plane"] / per_plane, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--planes", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join("profiles", "r16", "bench_contours.json"))
    a = ap.parse_args()
    import torch
    L = hip.lib()
    build = tempfile.mkdtemp()
    exe = os.path.join(build, "contour_host")
    subprocess.run(["g++", "-O2", "-std=c++17", "-o", exe,
                    os.path.join(REPO, "tests", "contour_host.cpp")], check=True)
    _, read_gbs = box_rates(L, a.warmup, a.reps)
    doc = {"tool": "bench_contours", "shape": [H, W], "flat_read_gb_per_s": round(read_gbs, 1),
           "trace": "lane 0 of the object's wave; the eight-lane probe was not built",
           "lds_pixels": hip.CONTOUR_LDS_PIXELS, "contents": []}
    for name, cells in (("voronoi_2000", 2000), ("voronoi_50000", 50000)):
        print("making %s" % name, file=sys.stderr, flush=True)
        distinct = [voronoi(cells, 100 + cells + k) for k in range(4)]
        planes = np.ascontiguousarray(np.stack([distinct[p % 4] for p in range(a.planes)]))
        doc["contents"].append(bench_content(L, torch, exe, name, planes, a.warmup, a.reps,
                                             read_gbs))
    doc["contents"].append(bench_content(L, torch, exe, "nested_rings",
                                         nested_rings()[None].copy(), a.warmup, a.reps, read_gbs))
    text = json.dumps(doc, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
