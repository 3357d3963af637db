#!/usr/bin/env python3
"""Times JPEG decoding of a pyramid's tiles on the synthetic channel layer of
tools/bench_pyramid.py (default: 384 wells of 3 x 3 sites of 2160 x 2560, 500 px
spacers = 3,456 sites) and prints one JSON line.  Per-kernel HIP-event times
of the library, warm-up and several repetitions in this one process:

* the JPEG round trip of the base level (``tmh_jpeg_roundtrip_level_device``);
* the pyramid's lower levels built with and without ``jpeg_quality`` (the
  halving passes, and the round trips between them);
* the decoder (``tmh_jpeg_decode_tiles_device``) over the base level's blob
  and over every level's;
* the encoder's measuring pass on the same base level;
* each next to the box's flat copy of the base level's bytes, taken in the
  same process (``tmh_box_probe_device`` mode 2);
* if Pillow imports, its decode rate on sampled base-level files over the
  granted cores (threads; libjpeg releases the GIL), the host comparison.

``--content cells`` or ``noise`` as in tools/bench_jpeg.py.

    python tools/bench_jpeg_decode.py [--wells 16x24] [--content cells] [--out FILE]
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
from bench_jpeg import site_image  # noqa: E402
from bench_pyramid import T, kernel_ms, layer, resident_sites  # noqa: E402
from tmlibrary_amd import hip  # noqa: E402
from tmlibrary_amd.workflow.pyramid import plan_base_tiles  # noqa: E402


def pillow_rate(files, threads):
    try:
        import io
        from concurrent.futures import ThreadPoolExecutor
        from PIL import Image
    except ImportError:
        return None

    def one(data):
        return np.asarray(Image.open(io.BytesIO(data))).shape[0]
    with ThreadPoolExecutor(threads) as ex:
        list(ex.map(one, files[:64]))
        t0 = time.perf_counter()
        list(ex.map(one, files))
        dt = time.perf_counter() - t0
    return {"tiles": len(files), "threads": threads, "seconds": round(dt, 3),
            "tiles_per_s": round(len(files) / dt, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--wells", default="16x24")
    ap.add_argument("--sites-per-side", type=int, default=3)
    ap.add_argument("--size", default="2160x2560")
    ap.add_argument("--spacer", type=int, default=500)
    ap.add_argument("--content", default="cells", choices=("cells", "noise"))
    ap.add_argument("--quality", type=int, default=95)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--pillow-tiles", type=int, default=2000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    wr, wc = (int(v) for v in a.wells.split("x"))
    H, W = (int(v) for v in a.size.split("x"))
    L = hip.lib()

    g = layer(wr, wc, a.sites_per_side, (H, W), a.spacer)
    n = len(g.sites)
    table = plan_base_tiles(g)
    rows, cols = g.dimensions[-1]
    site = site_image(a.content, H, W)
    d_sites = resident_sites(site, n)

    levels = [(rows, cols)]
    while levels[-1] != (1, 1):
        levels.append(((levels[-1][0] + 1) // 2, (levels[-1][1] + 1) // 2))
    d_levels = [hip.DeviceBuffer(r * c * T * T) for r, c in levels]
    level_b = rows * cols * T * T
    d_scratch = hip.DeviceBuffer(level_b)
    hip.check(L.tmh_tiles_base_device(d_sites, n, H, W, hip.ptr(table), len(table), d_levels[0],
                                      rows, cols, None))
    d_sites.free()

    def lower_levels(quality):
        """levels 1.. from the base, as build_pyramid queues them (a mosaic
        with an odd side is left to the host there; here its tile stays as
        the allocation holds it) -> the levels' last sizes"""
        lasts = [(T, T)]
        for z in range(len(levels) - 1):
            src = d_levels[z]
            if quality is not None:
                hip.check(L.tmh_jpeg_roundtrip_level_device(src, levels[z][0], levels[z][1],
                                                            lasts[z][0], lasts[z][1], quality,
                                                            d_scratch, None))
                src = d_scratch
            lh, lw = C.c_int(), C.c_int()
            hip.check(L.tmh_pyramid_shrink2_device(src, levels[z][0], levels[z][1], lasts[z][0],
                                                   lasts[z][1], d_levels[z + 1], C.byref(lh),
                                                   C.byref(lw), None))
            lasts.append((lh.value, lw.value))
        hip.check(L.tmh_synchronize(None))
        return lasts

    # the box's flat copy of the base level's bytes (read them once, write them once)
    npx = 1 << 20
    probe_sites = level_b // (2 * npx)
    ptrs = np.array([d_levels[0].ptr.value, d_scratch.ptr.value], dtype=np.uint64)
    copy_ms = C.c_double()
    with hip.DeviceBuffer.from_array(ptrs) as d_ptrs:
        for reps in (a.warmup, a.reps):
            hip.check(L.tmh_box_probe_device(d_ptrs, d_ptrs.at(8), 24, probe_sites, 1024, 1024, 2,
                                             reps, None, C.byref(copy_ms), None))
    copy_ms = copy_ms.value * level_b / (probe_sites * 2 * npx)

    hip.check(L.tmh_profile_enable(1))

    def timed(names, call):
        for rep in range(a.warmup + a.reps):
            if rep == a.warmup:
                hip.check(L.tmh_profile_reset())
            out = call()
        hip.check(L.tmh_synchronize(None))
        ms = {}
        for name in names:
            t, k = kernel_ms(L, name)
            assert k % a.reps == 0, (name, k)
            ms[name] = t / a.reps
        return ms, out

    rt, _ = timed(["jpeg_roundtrip"], lambda: hip.check(L.tmh_jpeg_roundtrip_level_device(
        d_levels[0], rows, cols, T, T, a.quality, d_scratch, None)))
    plain, _ = timed(["pyramid_shrink2"], lambda: lower_levels(None))
    stored, lasts = timed(["pyramid_shrink2", "jpeg_roundtrip"], lambda: lower_levels(a.quality))

    # the stored pyramid's files, level by level; the decoder over them
    decode_levels, base_files, measure_ms = [], None, None
    for z, (r, c) in enumerate(levels):
        nt = r * c
        d_off = hip.DeviceBuffer((nt + 1) * 8)
        total = C.c_int64()
        args = (d_levels[z], r, c, lasts[z][0], lasts[z][1], a.quality)
        if z == 0:
            m, _ = timed(["jpeg_measure"], lambda: hip.check(L.tmh_jpeg_encode_level_device(
                *args, None, 0, d_off, C.byref(total), None)))
            measure_ms = m["jpeg_measure"]
        hip.check(L.tmh_jpeg_encode_level_device(*args, None, 0, d_off, C.byref(total), None))
        d_blob = hip.DeviceBuffer(total.value)
        hip.check(L.tmh_jpeg_encode_level_device(*args, d_blob, total.value, d_off, C.byref(total),
                                                 None))
        d_dims, d_status = hip.DeviceBuffer(nt * 8), hip.DeviceBuffer(nt * 4)
        # decoded into the scratch level: the base level's size at the most
        ms, _ = timed(["jpeg_decode_tiles"], lambda: hip.check(L.tmh_jpeg_decode_tiles_device(
            d_blob, d_off, nt, d_scratch, d_dims, d_status, None)))
        assert not d_status.get(nt, np.int32).any(), "a file of level %d was not decoded" % z
        decode_levels.append({"tiles": [r, c], "last": list(lasts[z]),
                              "decode_ms": round(ms["jpeg_decode_tiles"], 4),
                              "tiles_per_s": round(nt / ms["jpeg_decode_tiles"] * 1e3, 1),
                              "input_bytes": int(total.value)})
        if z == 0 and a.pillow_tiles > 0:
            offsets = d_off.get(nt + 1, np.int64)
            pick = np.sort(np.random.default_rng(1).choice(nt, min(a.pillow_tiles, nt), replace=False))
            base_files = [d_blob.get(int(offsets[t + 1] - offsets[t]), np.uint8,
                                     int(offsets[t])).tobytes() for t in pick]
        for buf in (d_off, d_blob, d_dims, d_status):
            buf.free()
    hip.check(L.tmh_profile_enable(0))

    pillow = pillow_rate(base_files, min(16, os.cpu_count() or 1)) if base_files else None
    all_ms = sum(p["decode_ms"] for p in decode_levels)
    all_tiles = sum(r * c for r, c in levels)
    of_copy = lambda ms: round(ms / copy_ms, 2)  # noqa: E731
    stored_ms = stored["pyramid_shrink2"] + stored["jpeg_roundtrip"]
    result = {
        "bench": "jpeg_decode", "content": a.content, "quality": a.quality, "sites": n,
        "site_size": [H, W], "wells": [wr, wc], "spacer": a.spacer, "warmup": a.warmup,
        "reps": a.reps, "base_tiles": [rows, cols],
        "empty_base_tiles": round(len(g.get_empty_base_tile_coordinates()) / (rows * cols), 4),
        "flat_copy_of_base_level": {"bytes": level_b, "ms": round(copy_ms, 4)},
        "roundtrip_base": {"ms": round(rt["jpeg_roundtrip"], 4), "of_flat_copy": of_copy(rt["jpeg_roundtrip"]),
                           "tiles_per_s": round(rows * cols / rt["jpeg_roundtrip"] * 1e3, 1)},
        "encoder_measure_base": {"ms": round(measure_ms, 4), "of_flat_copy": of_copy(measure_ms)},
        "lower_levels": {
            "plain": {"shrink_ms": round(plain["pyramid_shrink2"], 4),
                      "of_flat_copy": of_copy(plain["pyramid_shrink2"])},
            "stored": {"shrink_ms": round(stored["pyramid_shrink2"], 4),
                       "roundtrip_ms": round(stored["jpeg_roundtrip"], 4),
                       "ms": round(stored_ms, 4), "of_flat_copy": of_copy(stored_ms)}},
        "decode_base": dict(decode_levels[0], of_flat_copy=of_copy(decode_levels[0]["decode_ms"])),
        "decode_all_levels": {"tiles": all_tiles, "decode_ms": round(all_ms, 4),
                              "tiles_per_s": round(all_tiles / all_ms * 1e3, 1),
                              "input_bytes": sum(p["input_bytes"] for p in decode_levels)},
        "decode_levels": decode_levels,
        "pillow_decode": pillow,
    }
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
