#!/usr/bin/env python3
"""Times jterator's site I/O kernels and writes one JSON document (default
profiles/r13/bench_jterator.json):

(a) the channel stack (tmh_correct_stack_u16_device): 64 sites x 4 channels of
    2160 x 2560 with ``slots`` 1 and 4, shifts within +-20 -- per channel call
    the library's HIP-event time of the stack launch and its fixup ("stack"),
    against the box's flat copy (``tmh_box_probe_device`` mode 2, same
    process) of the bytes the stack reads from the sites and writes, and the
    wall time of the call plus the download of the stack against the present
    route: tmh_correct_u16_device + download + host crop and strided scatter;
(b) the object table (tmh_object_table_device): planes of 2160 x 2560 with
    about 2,000 and about 50,000 Voronoi cells and a checkerboard of two
    labels -- the HIP-event time of init + table + finalize ("objects") per
    plane against the box's flat read of the plane (mode 3), the whole call
    (label range pass and its wait included), and scipy.ndimage
    (find_objects + center_of_mass) on the granted cores.

    python tools/bench_jterator.py [--sites 64] [--out FILE]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench_pyramid import kernel_ms  # noqa: E402
from tmlibrary_amd import hip  # noqa: E402
from tmlibrary_amd.image import Corrector, align_window  # noqa: E402
from tmlibrary_amd.models.file import granted_cores  # noqa: E402

H, W = 2160, 2560


def box_rates(L, warmup, reps):
    """(copy GB/s counting bytes read + written, read GB/s) of the flat probe."""
    npx, probe_sites = 1 << 20, 128
    out = []
    with hip.DeviceBuffer(probe_sites * npx * 2) as d_a, \
            hip.DeviceBuffer(probe_sites * npx * 2) as d_b:
        ptrs = np.array([d_a.ptr.value, d_b.ptr.value], dtype=np.uint64)
        with hip.DeviceBuffer.from_array(ptrs) as d_ptrs:
            for mode, factor in ((2, 2), (3, 1)):
                ms = C.c_double()
                for n in (warmup, reps):
                    hip.check(L.tmh_box_probe_device(d_ptrs, d_ptrs.at(8), 24, probe_sites, 1024,
                                                     1024, mode, n, None, C.byref(ms), None))
                out.append(factor * probe_sites * npx * 2 / (ms.value * 1e6))
    return out


def stat_planes(channel):
    yy, xx = np.mgrid[0:H, 0:W]
    mean = 2.45 + 0.05 * channel + 0.15 * np.exp(-((yy - H / 2.0) ** 2 + (xx - W / 2.0) ** 2)
                                                 / (0.3 * H * W))
    std = 0.2 + 0.05 * (xx / float(W)) + 0.01 * channel
    return mean, std


def bench_stack(L, torch, sites, channels, Z, T, warmup, reps, copy_gbs):
    dev = torch.device("cuda", 0)
    slots = Z * T
    n_planes = sites * slots
    planes = torch.empty((n_planes, H, W), dtype=torch.int16, device=dev)
    hip.check(L.tmh_synth_sites_device(C.c_void_p(planes.data_ptr()), n_planes, H, W, 12345, 0, 0,
                                       0, None))
    hip.check(L.tmh_synchronize(None))
    rng = np.random.default_rng(2)
    ys, xs = rng.integers(-20, 21, sites), rng.integers(-20, 21, sites)
    top, bottom = int(max(ys.max(), 0)), int(max(-ys.min(), 0))
    left, right = int(max(xs.max(), 0)), int(max(-xs.min(), 0))
    right += (W - left - right) % 8  # aligned widths are not multiples of 8 by nature; the wide
    # form of slots == 1 needs one, and the site geometry decides it once per experiment
    site = np.repeat(np.arange(sites), slots).astype(np.int32)
    slot = np.tile(np.arange(slots), sites).astype(np.int32)
    win = np.zeros(n_planes, dtype=hip.WINDOW_DTYPE)
    for p in range(n_planes):
        w, extent = align_window((H, W), int(ys[site[p]]), int(xs[site[p]]), bottom, top, right,
                                 left, crop=True)
        win[p] = w
    oh, ow = extent
    out = torch.empty((sites, oh, ow, slots), dtype=torch.int16, device=dev)
    correctors = [Corrector(*stat_planes(ch)) for ch in range(channels)]

    def call(corr):
        hip.check(L.tmh_correct_stack_u16_device(
            corr._h, C.c_void_p(planes.data_ptr()), C.c_void_p(out.data_ptr()), n_planes, H, W,
            hip.ptr(site), hip.ptr(slot), hip.ptr(win), sites, slots, oh, ow, None))

    hip.check(L.tmh_profile_enable(0))
    for _ in range(warmup):
        for corr in correctors:
            call(corr)
    walls = []
    for _ in range(reps):
        for corr in correctors:
            t0 = time.perf_counter()
            call(corr)
            walls.append(time.perf_counter() - t0)
    hip.check(L.tmh_profile_enable(1))
    hip.check(L.tmh_profile_reset())
    for _ in range(reps):
        for corr in correctors:
            call(corr)
    ms, launches = kernel_ms(L, "stack")
    hip.check(L.tmh_profile_enable(0))
    per_call = ms / (reps * channels)
    moved = 2 * n_planes * oh * ow * 2  # site bytes read + stack bytes written
    flat = moved / (copy_gbs * 1e6)

    # one channel end to end: this route and the present one, stack on the host at the end
    corr = correctors[0]
    t0 = time.perf_counter()
    call(corr)
    new_host = out.cpu().numpy().view(np.uint16)
    new_wall = time.perf_counter() - t0
    tmp = torch.empty_like(planes)
    t0 = time.perf_counter()
    hip.check(L.tmh_correct_u16_device(corr._h, C.c_void_p(planes.data_ptr()),
                                       C.c_void_p(tmp.data_ptr()), n_planes, -1, -1, None))
    hip.check(L.tmh_synchronize(None))
    t1 = time.perf_counter()
    full = tmp.cpu().numpy().view(np.uint16)
    t2 = time.perf_counter()
    old_host = np.zeros((sites, oh, ow, Z, T), np.uint16)
    for p in range(n_planes):
        r0, c0 = int(win[p]["src_r0"]), int(win[p]["src_c0"])
        z, t = divmod(int(slot[p]), T)
        old_host[site[p], :, :, z, t] = full[p, r0:r0 + oh, c0:c0 + ow]
    t3 = time.perf_counter()
    same = bool(np.array_equal(old_host.reshape(new_host.shape), new_host))
    for c in correctors:
        c.close()
    return {"sites": sites, "channels": channels, "zplanes": Z, "tpoints": T, "slots": slots,
            "planes_per_channel": n_planes, "aligned_shape": [int(oh), int(ow)],
            "stack_kernel_ms_per_channel": round(per_call, 4),
            "stack_kernel_ms_all_channels": round(per_call * channels, 4),
            "launches_per_channel": launches // (reps * channels),
            "bytes_moved_per_channel": int(moved),
            "gb_per_s": round(moved / (per_call * 1e6), 1),
            "flat_copy_ms_per_channel": round(flat, 4),
            "x_flat_copy": round(per_call / flat, 2),
            "call_wall_ms_median": round(float(np.median(walls)) * 1e3, 3),
            "route_new_wall_ms": round(new_wall * 1e3, 1),
            "route_present_wall_ms": round((t3 - t0) * 1e3, 1),
            "route_present_parts_ms": {"correct_device": round((t1 - t0) * 1e3, 1),
                                       "download": round((t2 - t1) * 1e3, 1),
                                       "host_crop_scatter": round((t3 - t2) * 1e3, 1)},
            "route_gain": round((t3 - t0) / new_wall, 2),
            "routes_equal": same}


def voronoi(n_cells, seed):
    import scipy.ndimage as ndi
    rng = np.random.default_rng(seed)
    seeds = np.zeros((H, W), np.int32)
    seeds[rng.integers(0, H, n_cells), rng.integers(0, W, n_cells)] = 1
    ys, xs = np.nonzero(seeds)
    seeds[ys, xs] = np.arange(1, ys.size + 1, dtype=np.int32)
    idx = ndi.distance_transform_edt(seeds == 0, return_distances=False, return_indices=True)
    return np.ascontiguousarray(seeds[idx[0], idx[1]])


def scipy_rate(plane, threads):
    import scipy.ndimage as ndi
    from concurrent.futures import ThreadPoolExecutor
    labels = np.unique(plane[plane > 0])

    def one(_):
        ndi.find_objects(plane)
        ndi.center_of_mass(plane, plane, labels)
    with ThreadPoolExecutor(threads) as ex:
        t0 = time.perf_counter()
        list(ex.map(one, range(threads)))
        dt = time.perf_counter() - t0
    return {"planes": threads, "threads": threads, "seconds": round(dt, 3),
            "ms_per_plane": round(dt / threads * 1e3, 2)}


def bench_objects(L, torch, name, plane, n_planes, warmup, reps, read_gbs, threads):
    dev = torch.device("cuda", 0)
    d = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(plane, (n_planes, H, W)))).to(dev)
    top = int(plane.max())
    rows = torch.empty((n_planes * (top + 1) * 48,), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()

    def call():
        hip.check(L.tmh_object_table_device(C.c_void_p(d.data_ptr()), n_planes, H, W, top,
                                            C.c_void_p(rows.data_ptr()), None))
        hip.check(L.tmh_synchronize(None))

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
    ms, _ = kernel_ms(L, "objects")
    hip.check(L.tmh_profile_enable(0))
    got = rows.cpu().numpy().view(hip.OBJECT_ROW_DTYPE).reshape(n_planes, top + 1)
    counts = np.bincount(plane.reshape(-1), minlength=top + 1)
    ok = bool(all(np.array_equal(got[p]["n"], counts) for p in range(n_planes)))
    per_plane = ms / (reps * n_planes)
    flat = H * W * 4 / (read_gbs * 1e6)
    runs = int(np.count_nonzero(np.diff(plane, axis=1)) + H)
    out = {"content": name, "objects": int(np.count_nonzero(counts[1:])), "runs_per_plane": runs,
           "planes_per_call": n_planes, "counts_correct": ok,
           "table_kernels_ms_per_plane": round(per_plane, 4),
           "gb_per_s": round(H * W * 4 / (per_plane * 1e6), 1),
           "flat_read_ms_per_plane": round(flat, 4),
           "x_flat_read": round(per_plane / flat, 2),
           "call_wall_ms_per_plane": round(float(np.median(walls)) * 1e3 / n_planes, 4)}
    out["scipy_find_objects_center_of_mass"] = scipy_rate(plane, threads)
    out["x_scipy"] = round(out["scipy_find_objects_center_of_mass"]["ms_per_plane"]
                           / out["call_wall_ms_per_plane"], 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sites", type=int, default=64)
    ap.add_argument("--channels", type=int, default=4)
    ap.add_argument("--planes", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join("profiles", "r13", "bench_jterator.json"))
    a = ap.parse_args()
    import torch
    L = hip.lib()
    threads = max(1, min(16, granted_cores()))
    copy_gbs, read_gbs = box_rates(L, a.warmup, a.reps)
    doc = {"tool": "bench_jterator", "shape": [H, W], "flat_copy_gb_per_s": round(copy_gbs, 1),
           "flat_read_gb_per_s": round(read_gbs, 1), "threads": threads, "stack": [],
           "objects": []}
    for Z, T in ((1, 1), (2, 2)):
        doc["stack"].append(bench_stack(L, torch, a.sites, a.channels, Z, T, a.warmup, a.reps,
                                        copy_gbs))
    yy, xx = np.mgrid[0:H, 0:W]
    contents = (("voronoi_2000", voronoi(2000, 1)), ("voronoi_50000", voronoi(50000, 2)),
                ("checkerboard", ((yy + xx) % 2 + 1).astype(np.int32)))
    for name, plane in contents:
        doc["objects"].append(bench_objects(L, torch, name, plane, a.planes, a.warmup, a.reps,
                                            read_gbs, threads))
    text = json.dumps(doc, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
