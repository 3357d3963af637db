#!/usr/bin/env python3
"""Times the two pyramid kernels on a synthetic channel layer of resident
uint8 sites (default: 384 wells of 3 x 3 sites of 2160 x 2560, 500 px spacers
= 3,456 sites, 19 GB) and prints one JSON line:

* per-kernel HIP-event times (the library's per-kernel event timing), warm-up
  and several repetitions in this one process;
* the bytes each pass moves;
* for the base pass, its rate against the box's flat copy of the same byte
  count, taken in the same process (``tmh_box_probe_device`` mode 2) -- the
  pass reads and writes each byte once, so the copy is its yardstick.

    python tools/bench_pyramid.py [--wells 16x24] [--reps 5] [--out FILE]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tmlibrary_amd import hip  # noqa: E402
from tmlibrary_amd.workflow.pyramid import LayerGeometry, plan_base_tiles  # noqa: E402

T = 256


def layer(well_rows, well_cols, sites_per_side, size, spacer):
    H, W = size
    sites = []
    for wr in range(well_rows):
        for wc in range(well_cols):
            oy = wr * (sites_per_side * H + spacer)
            ox = wc * (sites_per_side * W + spacer)
            for y in range(sites_per_side):
                for x in range(sites_per_side):
                    sites.append((wr * well_cols + wc, y, x, (oy + y * H, ox + x * W)))
    dims = {w: (sites_per_side, sites_per_side) for w in range(well_rows * well_cols)}
    return LayerGeometry(size, sites, dims)


def resident_sites(site, n):
    """n copies of one host site, back to back in a ``hip.DeviceBuffer``."""
    d_sites = hip.DeviceBuffer(n * site.nbytes)
    for i in range(n):
        d_sites.put(site, i * site.nbytes)
    return d_sites


def kernel_ms(L, name):
    ms, n = C.c_double(), C.c_int64()
    hip.check(L.tmh_profile_read(name.encode(), C.byref(ms), C.byref(n)))
    return ms.value, n.value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--wells", default="16x24")
    ap.add_argument("--sites-per-side", type=int, default=3)
    ap.add_argument("--size", default="2160x2560")
    ap.add_argument("--spacer", type=int, default=500)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    wr, wc = (int(v) for v in a.wells.split("x"))
    H, W = (int(v) for v in a.size.split("x"))
    L = hip.lib()

    g = layer(wr, wc, a.sites_per_side, (H, W), a.spacer)
    n = len(g.sites)
    t0 = time.perf_counter()
    table = plan_base_tiles(g)
    plan_s = time.perf_counter() - t0
    rows, cols = g.dimensions[-1]
    read_b = int((table["height"].astype(np.int64) * table["width"]).sum())
    write_b = rows * cols * T * T

    # resident sites: one random site, uploaded n times
    site = np.random.default_rng(0).integers(0, 256, (H, W), dtype=np.uint8)
    d_sites = resident_sites(site, n)

    levels = [(rows, cols)]
    while levels[-1] != (1, 1):
        levels.append(((levels[-1][0] + 1) // 2, (levels[-1][1] + 1) // 2))
    d_levels = [hip.DeviceBuffer(r * c * T * T) for r, c in levels]

    # the box's flat copy of the base pass's byte count: (read + write) / 2 each way
    npx = 1 << 20
    probe_sites = max(1, (read_b + write_b) // 2 // (2 * npx))
    assert probe_sites * 2 * npx <= write_b
    d_probe_out = hip.DeviceBuffer(probe_sites * 2 * npx)
    ptrs = np.array([d_levels[0].ptr.value, d_probe_out.ptr.value], dtype=np.uint64)
    d_ptrs = hip.DeviceBuffer.from_array(ptrs)
    copy_ms = C.c_double()
    hip.check(L.tmh_box_probe_device(d_ptrs, d_ptrs.at(8), 24, probe_sites, 1024,
                                     1024, 2, a.warmup, None, C.byref(copy_ms), None))
    hip.check(L.tmh_box_probe_device(d_ptrs, d_ptrs.at(8), 24, probe_sites, 1024,
                                     1024, 2, a.reps, None, C.byref(copy_ms), None))
    copy_bytes = probe_sites * 2 * npx * 2
    copy_gbs = copy_bytes / copy_ms.value / 1e6
    d_probe_out.free()

    hip.check(L.tmh_profile_enable(1))
    for rep in range(a.warmup + a.reps):
        if rep == a.warmup:
            hip.check(L.tmh_profile_reset())
        hip.check(L.tmh_tiles_base_device(d_sites, n, H, W, hip.ptr(table), len(table),
                                          d_levels[0], rows, cols, None))
    ms, launches = kernel_ms(L, "tiles_base")
    assert launches == a.reps
    ms /= launches
    gbs = (read_b + write_b) / ms / 1e6
    # (keyed as in earlier rounds' lines, which also timed a retired aligned-pair form)
    base = {"unaligned": {"ms": round(ms, 4), "gb_per_s": round(gbs, 1),
                          "of_flat_copy": round(gbs / copy_gbs, 4)}}

    shrink = []
    last = (T, T)
    for z in range(len(levels) - 1):
        r, c = levels[z]
        lh, lw = C.c_int(), C.c_int()
        for rep in range(a.warmup + a.reps):
            if rep == a.warmup:
                hip.check(L.tmh_profile_reset())
            hip.check(L.tmh_pyramid_shrink2_device(d_levels[z], r, c, last[0], last[1],
                                                   d_levels[z + 1], C.byref(lh), C.byref(lw), None))
        hip.check(L.tmh_synchronize(None))
        ms, launches = kernel_ms(L, "pyramid_shrink2")
        ms /= launches
        moved = (r * c + levels[z + 1][0] * levels[z + 1][1]) * T * T
        shrink.append({"src_tiles": [r, c], "last": list(last), "ms": round(ms, 4),
                       "bytes": moved, "gb_per_s": round(moved / ms / 1e6, 1)})
        last = (lh.value, lw.value)
    hip.check(L.tmh_profile_enable(0))

    result = {
        "bench": "pyramid", "sites": n, "site_size": [H, W], "wells": [wr, wc],
        "spacer": a.spacer, "base_tiles": [rows, cols], "rectangles": int(len(table)),
        "plan_seconds": round(plan_s, 2), "warmup": a.warmup, "reps": a.reps,
        "base_read_bytes": read_b, "base_write_bytes": write_b,
        "flat_copy": {"bytes": copy_bytes, "ms": round(copy_ms.value, 4),
                      "gb_per_s": round(copy_gbs, 1)},
        "tiles_base": base,
        "shrink_levels": shrink,
        "shrink_total_ms": round(sum(s["ms"] for s in shrink), 4),
        "shrink_total_bytes": sum(s["bytes"] for s in shrink),
    }
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
