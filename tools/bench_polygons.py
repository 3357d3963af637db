#!/usr/bin/env python3
"""Label planes from outlines at full size on one MI355X.

Per content -- 16 planes of 2160 x 2560 whose outlines are the outer borders
``tmh_object_contours`` traces on Voronoi planes of about 2,000 and about
50,000 cells (four distinct planes, each four times), and one plane with a
single plane-sized ring, whose box takes the memory route:
  * ``tmh_polygon_fill_device``: HIP-event time of zeroing, drawing and the
    index -> label pass per plane (``tmh_profile_read("polygons")``), the wall
    time of the call (which adds the checks of the lists and their waits), and
    the ratio to a flat write of the plane at the box's copy rate
    (``tmh_box_probe_device`` mode 2, bytes read + written; the probe has no
    write-only mode);
  * the host core -- tests/polygon_host.cpp over polygon_core.h, ``g++ -O2``,
    the same toggles and suffix XOR -- on sixteen processes, one plane's rings
    each.  scikit-image is not installed here, so the host core stands in for
    the reference's loop; it is O(vertices + area / 64) where the reference
    tests every pixel against every vertex, and leaves out its Python;
  * plane 0 of the device result checked against the host core's output.

    python tools/bench_polygons.py [--out profiles/r19/bench_polygons.json]
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
from tmlibrary_amd.image import object_contours  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROCESSES = 16


def outlines(plane):
    """(labels, first, points) of a label plane's outer borders as stored
    rings: global (x, y) with y negated, offsets 0."""
    rows, objects, contours, points = object_contours(plane[None])
    outer = np.nonzero(contours["is_hole"] == 0)[0]
    c = contours[outer]
    r = rows[0][c["label"]]
    n = c["n_points"].astype(np.int64)
    first = np.zeros(len(c) + 1, np.int64)
    np.cumsum(n, out=first[1:])
    idx = np.repeat(c["point_offset"] - first[:-1], n) + np.arange(first[-1])
    pts = points[idx].astype(np.int64)
    pts[:, 0] += np.repeat(r["x0"].astype(np.int64) - 1, n)
    pts[:, 1] += np.repeat(r["y0"].astype(np.int64) - 1, n)
    pts[:, 1] *= -1
    return c["label"].astype(np.int32), first, np.ascontiguousarray(pts.astype(np.int32))


def plane_ring():
    pts = np.array([[0, 0], [W - 1, -40], [W - 60, -(H - 1)], [30, -(H - 20)]], np.int32)
    return np.array([1], np.int32), np.array([0, 4], np.int64), pts


def stacked(per_plane, n_planes):
    """The lists of n_planes planes, plane p drawing per_plane[p % len]."""
    labels, firsts, points, planes, at = [], [np.zeros(1, np.int64)], [], [], 0
    for p in range(n_planes):
        lab, first, pts = per_plane[p % len(per_plane)]
        labels.append(lab)
        firsts.append(first[1:] + at)
        at += first[-1]
        points.append(pts)
        planes.append(np.full(len(lab), p, np.int32))
    return (np.concatenate(points), np.concatenate(firsts), np.concatenate(planes),
            np.concatenate(labels))


def write_case(path, lab, first, pts):
    with open(path, "wb") as f:
        f.write(np.array([1, H, W, len(lab)], np.int32).tobytes())
        f.write(np.array([0, 0], np.int64).tobytes())
        for k in range(len(lab)):
            ring = pts[first[k]:first[k + 1]]
            f.write(np.array([lab[k], len(ring)], np.int32).tobytes())
            f.write(ring.tobytes())


def host_core(exe, tmp, lab, first, pts):
    src = os.path.join(tmp, "case")
    write_case(src, lab, first, pts)
    t0 = time.perf_counter()
    procs = [subprocess.Popen([exe, src, os.path.join(tmp, "out%d" % i)]) for i in range(PROCESSES)]
    codes = [p.wait() for p in procs]
    dt = time.perf_counter() - t0
    assert not any(codes), codes
    stats = {"processes": PROCESSES, "planes": PROCESSES, "seconds": round(dt, 3),
             "ms_per_plane": round(dt / PROCESSES * 1e3, 2),
             "note": "polygon_host (g++ -O2) stands in for skimage.draw.polygon, which is not "
                     "installed; it reads its rings from a file and writes the plane to one"}
    return stats, np.fromfile(os.path.join(tmp, "out0"), np.int32).reshape(H, W)


def bench_content(L, torch, exe, name, per_plane, n_planes, warmup, reps, copy_gbs):
    dev = torch.device("cuda", 0)
    points, first, plane, label = stacked(per_plane, n_planes)
    d = [torch.from_numpy(a.reshape(-1).view(np.uint8).copy()).to(dev)
         for a in (points, first, plane, label)]
    out = torch.empty((n_planes, H, W), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    P = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731

    def call():
        hip.check(L.tmh_polygon_fill_device(P(d[0]), P(d[1]), P(d[2]), P(d[3]), len(label),
                                            n_planes, H, W, 0, 0, P(out), None))

    hip.check(L.tmh_profile_enable(0))
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
    ms, _ = kernel_ms(L, "polygons")
    hip.check(L.tmh_profile_enable(0))
    got = out[0].cpu().numpy()
    print("%s: device done, host core" % name, file=sys.stderr, flush=True)
    with tempfile.TemporaryDirectory() as tmp:
        host, want = host_core(exe, tmp, *per_plane[0])
    per = ms / (reps * n_planes)
    flat = H * W * 4 / (copy_gbs * 1e6)
    return {"content": name, "planes_per_call": n_planes,
            "polygons_per_plane": int(len(per_plane[0][0])),
            "vertices_per_plane": int(per_plane[0][1][-1]),
            "filled_share_plane0": round(float((got != 0).mean()), 4),
            "fill_ms_per_plane": round(per, 4),
            "flat_write_ms_per_plane": round(flat, 4),
            "x_flat_write": round(per / flat, 1),
            "call_wall_ms_per_plane": round(float(np.median(walls)) * 1e3 / n_planes, 4),
            "equals_host_core_plane0": bool(np.array_equal(got, want)),
            "host_core": host,
            "x_host_core": round(host["ms_per_plane"] / per, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--planes", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join("profiles", "r19", "bench_polygons.json"))
    a = ap.parse_args()
    import torch
    L = hip.lib()
    build = tempfile.mkdtemp()
    exe = os.path.join(build, "polygon_host")
    subprocess.run(["g++", "-O2", "-std=c++17", "-o", exe,
                    os.path.join(REPO, "tests", "polygon_host.cpp")], check=True)
    copy_gbs, _ = box_rates(L, a.warmup, a.reps)
    doc = {"tool": "bench_polygons", "shape": [H, W], "flat_copy_gb_per_s": round(copy_gbs, 1),
           "lds_words": hip.POLYGON_LDS_WORDS, "contents": []}
    for name, cells in (("outlines_2000", 2000), ("outlines_50000", 50000)):
        print("making %s" % name, file=sys.stderr, flush=True)
        per_plane = [outlines(voronoi(cells, 100 + cells + k)) for k in range(4)]
        doc["contents"].append(bench_content(L, torch, exe, name, per_plane, a.planes, a.warmup,
                                             a.reps, copy_gbs))
    doc["contents"].append(bench_content(L, torch, exe, "plane_ring", [plane_ring()], a.planes,
                                         a.warmup, a.reps, copy_gbs))
    text = json.dumps(doc, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
