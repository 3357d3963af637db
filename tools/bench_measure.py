#!/usr/bin/env python3
"""Times the intensity measurement (tmh_intensity_table_device +
tmh_intensity_features_device) and writes one JSON document (default
profiles/r22/bench_measure.json).

16 planes of 2160 x 2560 with about 2,000 and about 50,000 Voronoi cells and a
checkerboard of two labels; 1 and 4 uint16 channels; the plain layout
[channel][plane][H][W] and the channel stack's layout [site][h][w][slot] with
4 slots, of which slot 0 of each site is read through strides.  Per case the
HIP-event time per plane of init + table + fix ("intensity") plus the finalize
("intensity_features"), against
  * the box's flat read (tmh_box_probe_device mode 3, same process) of the
    bytes the call must read: the labels once plus each channel once;
  * the object table on the same planes in the same process;
  * four one-channel calls, for the four-channel cases;
  * scipy.ndimage (sum, minimum, maximum, standard_deviation with labels=) on
    sixteen host processes, one plane and channel each, started before the
    GPU is opened.

    python tools/bench_measure.py [--planes 16] [--out FILE]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import multiprocessing
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench_jterator import H, W, box_rates, voronoi  # noqa: E402
from bench_pyramid import kernel_ms  # noqa: E402
from tmlibrary_amd import hip  # noqa: E402

_PLANE = None


def _scipy_one(seed):
    import scipy.ndimage as ndi
    plane = _PLANE
    img = np.random.default_rng(seed).integers(0, 65536, plane.shape).astype(np.uint16)
    index = np.unique(plane[plane > 0])
    t0 = time.perf_counter()
    ndi.sum(img, plane, index)
    ndi.minimum(img, plane, index)
    ndi.maximum(img, plane, index)
    ndi.standard_deviation(img, plane, index)
    return time.perf_counter() - t0


def scipy_rate(plane, procs):
    """procs processes (forked before the GPU is opened), one plane and channel each"""
    global _PLANE
    _PLANE = plane
    with multiprocessing.get_context("fork").Pool(procs) as pool:
        t0 = time.perf_counter()
        each = pool.map(_scipy_one, range(procs))
        dt = time.perf_counter() - t0
    return {"processes": procs, "plane_channels": procs, "seconds": round(dt, 3),
            "ms_per_plane_channel": round(dt / procs * 1e3, 2),
            "ms_in_scipy_per_plane_channel_one_process": round(float(np.median(each)) * 1e3, 1)}


def timed(L, call, names, warmup, reps):
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
    ms = {name: kernel_ms(L, name)[0] / reps for name in names}
    hip.check(L.tmh_profile_enable(0))
    return ms, float(np.median(walls)) * 1e3


def bench_case(L, torch, name, plane, n_planes, n_c, layout, warmup, reps, read_gbs, object_ms):
    dev = torch.device("cuda", 0)
    d_lab = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(plane, (n_planes, H, W)))).to(dev)
    top = int(plane.max())
    slots = 4 if layout == "stack" else 1
    g = torch.Generator(device=dev)
    g.manual_seed(5)
    # [channel][site][h][w][slot]: slots == 1 is the plain layout
    pix = torch.randint(0, 32768, (n_c, n_planes, H, W, slots), dtype=torch.int16, device=dev,
                        generator=g)
    n_rows = n_planes * (top + 1) * n_c
    rows = torch.empty((n_rows * 32,), dtype=torch.uint8, device=dev)
    obj = torch.empty((n_planes * (top + 1) * 48,), dtype=torch.uint8, device=dev)
    feat = torch.empty((n_rows * 5,), dtype=torch.float64, device=dev)
    hip.check(L.tmh_object_table_device(C.c_void_p(d_lab.data_ptr()), n_planes, H, W, top,
                                        C.c_void_p(obj.data_ptr()), None))
    torch.cuda.synchronize()
    strides = (n_planes * H * W * slots, H * W * slots, W * slots, slots)

    def table(c0, channels, row_at):
        hip.check(L.tmh_intensity_table_device(
            C.c_void_p(d_lab.data_ptr()), C.c_void_p(pix.data_ptr() + 2 * c0 * strides[0]), 2,
            n_planes, H, W, channels, *strides, top, C.c_void_p(obj.data_ptr()),
            C.c_void_p(rows.data_ptr() + row_at), None))

    def call():
        table(0, n_c, 0)
        hip.check(L.tmh_intensity_features_device(C.c_void_p(rows.data_ptr()), n_planes, n_planes,
                                                  top, n_c, C.c_void_p(feat.data_ptr()), None))
        hip.check(L.tmh_synchronize(None))

    ms, wall = timed(L, call, ("intensity", "intensity_features"), warmup, reps)
    got = rows.cpu().numpy().view(hip.INTENSITY_ROW_DTYPE).reshape(n_planes, top + 1, n_c)
    counts = np.bincount(plane.reshape(-1), minlength=top + 1)
    want_sum = np.bincount(plane.reshape(-1), weights=pix[0, 0, :, :, 0].cpu().numpy()
                           .astype(np.float64).reshape(-1), minlength=top + 1)
    ok = bool(np.array_equal(got[0, :, 0]["n"], counts)
              and np.array_equal(got[0, :, 0]["sum"].astype(np.float64), want_sum))
    per_plane = (ms["intensity"] + ms["intensity_features"]) / n_planes
    must_read = H * W * (4 + 2 * n_c)
    flat = must_read / (read_gbs * 1e6)
    out = {"content": name, "channels": n_c, "layout": layout,
           "objects": int(np.count_nonzero(counts[1:])),
           "runs_per_plane": int(np.count_nonzero(np.diff(plane, axis=1)) + H),
           "planes_per_call": n_planes, "n_and_sum_correct": ok,
           "table_ms_per_plane": round(ms["intensity"] / n_planes, 4),
           "finalize_ms_per_plane": round(ms["intensity_features"] / n_planes, 4),
           "ms_per_plane": round(per_plane, 4),
           "bytes_the_call_must_read_per_plane": must_read,
           "gb_per_s": round(must_read / (per_plane * 1e6), 1),
           "flat_read_ms_per_plane": round(flat, 4), "x_flat_read": round(per_plane / flat, 2),
           "object_table_ms_per_plane": round(object_ms, 4),
           "x_object_table": round(per_plane / object_ms, 2),
           "call_wall_ms_per_plane": round(wall / n_planes, 4)}
    if n_c > 1:
        def singles():
            for c in range(n_c):
                table(c, 1, 0)
            hip.check(L.tmh_synchronize(None))
        ms1, _ = timed(L, singles, ("intensity",), warmup, reps)
        out["one_channel_calls_table_ms_per_plane"] = round(ms1["intensity"] / n_planes, 4)
        out["x_one_channel_calls"] = round(ms1["intensity"] / ms["intensity"], 2)
    return out


def object_table_ms(L, torch, plane, n_planes, warmup, reps):
    dev = torch.device("cuda", 0)
    d = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(plane, (n_planes, H, W)))).to(dev)
    top = int(plane.max())
    rows = torch.empty((n_planes * (top + 1) * 48,), dtype=torch.uint8, device=dev)

    def call():
        hip.check(L.tmh_object_table_device(C.c_void_p(d.data_ptr()), n_planes, H, W, top,
                                            C.c_void_p(rows.data_ptr()), None))
        hip.check(L.tmh_synchronize(None))
    ms, _ = timed(L, call, ("objects",), warmup, reps)
    return ms["objects"] / n_planes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--planes", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--processes", type=int, default=16)
    ap.add_argument("--out", default=os.path.join("profiles", "r22", "bench_measure.json"))
    a = ap.parse_args()
    yy, xx = np.mgrid[0:H, 0:W]
    contents = (("voronoi_2000", voronoi(2000, 1)), ("voronoi_50000", voronoi(50000, 2)),
                ("checkerboard", ((yy + xx) % 2 + 1).astype(np.int32)))
    scipy = {name: scipy_rate(plane, a.processes) for name, plane in contents}   # before the GPU
    import torch
    L = hip.lib()
    _, read_gbs = box_rates(L, a.warmup, a.reps)
    doc = {"tool": "bench_measure", "shape": [H, W], "flat_read_gb_per_s": round(read_gbs, 1),
           "warmup": a.warmup, "reps": a.reps, "cases": [], "scipy_ndimage": scipy}
    for name, plane in contents:
        obj_ms = object_table_ms(L, torch, plane, a.planes, a.warmup, a.reps)
        for layout in ("plain", "stack"):
            for n_c in (1, 4):
                case = bench_case(L, torch, name, plane, a.planes, n_c, layout, a.warmup, a.reps,
                                  read_gbs, obj_ms)
                case["x_scipy"] = round(scipy[name]["ms_per_plane_channel"] * n_c
                                        / case["call_wall_ms_per_plane"], 1)
                doc["cases"].append(case)
                torch.cuda.empty_cache()
    text = json.dumps(doc, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
