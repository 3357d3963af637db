#!/usr/bin/env python3
"""Times the JPEG coding of a pyramid's tiles (tmh_jpeg_encode_level_device) on
the synthetic channel layer of tools/bench_pyramid.py (default: 384 wells of
3 x 3 sites of 2160 x 2560, 500 px spacers = 3,456 sites) and prints one JSON
line:

* per level and summed: the measuring pass and the writing pass (per-kernel
  HIP-event times of the library, warm-up and several repetitions in this one
  process), tiles/s, output bytes, the share of 1,100-byte files (all-zero
  tiles; any tile of one value gives a file of about that size);
* for the base level, the time against the box's flat copy of the level's
  bytes, taken in the same process (``tmh_box_probe_device`` mode 2);
* if Pillow imports, its encode rate on sampled base tiles over the granted
  cores (threads; libjpeg releases the GIL), the host comparison.

The sites are one image replicated: ``--content cells`` (blurred lognormal
blobs and a little noise, what a stained well looks like) or ``noise``
(uniform noise: the largest files an 8-bit tile gives).

    python tools/bench_jpeg.py [--wells 16x24] [--content cells] [--out FILE]
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
from bench_pyramid import T, kernel_ms, layer, resident_sites  # noqa: E402
from tmlibrary_amd import hip  # noqa: E402
from tmlibrary_amd.workflow.pyramid import plan_base_tiles  # noqa: E402


def site_image(content, H, W):
    rng = np.random.default_rng(0)
    if content == "noise":
        return rng.integers(0, 256, (H, W), dtype=np.uint8)
    a = np.zeros((H, W))
    n = H * W // 4000
    a[rng.integers(0, H, n), rng.integers(0, W, n)] = rng.lognormal(8.0, 0.6, n)
    fy, fx = np.fft.fftfreq(H)[:, None], np.fft.rfftfreq(W)[None, :]
    blur = np.exp(-2.0 * (np.pi * 7.0) ** 2 * (fy * fy + fx * fx))     # sigma 7 px
    a = np.fft.irfft2(np.fft.rfft2(a) * blur, s=(H, W))
    return np.clip(a + rng.normal(6.0, 1.5, (H, W)), 0, 255).astype(np.uint8)


def pillow_rate(tiles, threads, quality):
    try:
        import io
        from concurrent.futures import ThreadPoolExecutor
        from PIL import Image
    except ImportError:
        return None

    def one(a):
        buf = io.BytesIO()
        Image.fromarray(a, "L").save(buf, "JPEG", quality=quality)
        return buf.tell()
    with ThreadPoolExecutor(threads) as ex:
        list(ex.map(one, tiles[:64]))
        t0 = time.perf_counter()
        nbytes = sum(ex.map(one, tiles))
        dt = time.perf_counter() - t0
    return {"tiles": len(tiles), "threads": threads, "seconds": round(dt, 3),
            "tiles_per_s": round(len(tiles) / dt, 1), "bytes": int(nbytes)}


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
    lasts = [(T, T)]
    hip.check(L.tmh_tiles_base_device(d_sites, n, H, W, hip.ptr(table), len(table), d_levels[0],
                                      rows, cols, None))
    d_sites.free()
    for z in range(len(levels) - 1):
        lh, lw = C.c_int(), C.c_int()
        hip.check(L.tmh_pyramid_shrink2_device(d_levels[z], levels[z][0], levels[z][1], lasts[z][0],
                                               lasts[z][1], d_levels[z + 1], C.byref(lh),
                                               C.byref(lw), None))
        lasts.append((lh.value, lw.value))
        # (the device pass leaves a mosaic with an odd side to the host; here such a tile is
        # coded as the allocation holds it)
    hip.check(L.tmh_synchronize(None))

    # the box's flat copy of the base level's bytes (read them once, write them once)
    level_b = rows * cols * T * T
    npx = 1 << 20
    probe_sites = level_b // (2 * npx)
    copy_ms = C.c_double()
    with hip.DeviceBuffer(probe_sites * 2 * npx) as d_probe_out:
        ptrs = np.array([d_levels[0].ptr.value, d_probe_out.ptr.value], dtype=np.uint64)
        with hip.DeviceBuffer.from_array(ptrs) as d_ptrs:
            for reps in (a.warmup, a.reps):
                hip.check(L.tmh_box_probe_device(d_ptrs, d_ptrs.at(8), 24, probe_sites, 1024, 1024,
                                                 2, reps, None, C.byref(copy_ms), None))
    copy_ms = copy_ms.value * level_b / (probe_sites * 2 * npx)

    hip.check(L.tmh_profile_enable(1))
    per_level = []
    for z, (r, c) in enumerate(levels):
        nt = r * c
        total = C.c_int64()
        d_off = hip.DeviceBuffer((nt + 1) * 8)
        hip.check(L.tmh_jpeg_encode_level_device(d_levels[z], r, c, lasts[z][0], lasts[z][1],
                                                 a.quality, None, 0, d_off, C.byref(total), None))
        d_out = hip.DeviceBuffer(total.value)
        for rep in range(a.warmup + a.reps):
            if rep == a.warmup:
                hip.check(L.tmh_profile_reset())
            hip.check(L.tmh_jpeg_encode_level_device(d_levels[z], r, c, lasts[z][0], lasts[z][1],
                                                     a.quality, d_out, total.value, d_off,
                                                     C.byref(total), None))
        m_ms, m_n = kernel_ms(L, "jpeg_measure")
        w_ms, w_n = kernel_ms(L, "jpeg_write")
        assert m_n == w_n == a.reps
        offsets = d_off.get(nt + 1, np.int64)
        m_ms, w_ms = m_ms / m_n, w_ms / w_n
        per_level.append({
            "tiles": [r, c], "last": list(lasts[z]), "measure_ms": round(m_ms, 4),
            "write_ms": round(w_ms, 4), "writing_call_ms": round(m_ms + w_ms, 4),
            "tiles_per_s": round(nt / (m_ms + w_ms) * 1e3, 1), "output_bytes": int(total.value),
            "files_of_1100_bytes": round(float(np.mean(np.diff(offsets) == 1100)), 4)})
        d_off.free()
        d_out.free()
    hip.check(L.tmh_profile_enable(0))

    pillow = None
    if a.pillow_tiles > 0:
        pick = np.sort(np.random.default_rng(1).choice(rows * cols, min(a.pillow_tiles, rows * cols),
                                                       replace=False))
        tiles = [d_levels[0].get((T, T), np.uint8, int(t) * T * T) for t in pick]
        pillow = pillow_rate(tiles, min(16, os.cpu_count() or 1), a.quality)

    base = per_level[0]
    all_ms = sum(p["writing_call_ms"] for p in per_level)
    all_tiles = sum(r * c for r, c in levels)
    result = {
        "bench": "jpeg", "content": a.content, "quality": a.quality, "sites": n,
        "site_size": [H, W], "wells": [wr, wc], "spacer": a.spacer, "warmup": a.warmup,
        "reps": a.reps, "base_tiles": [rows, cols],
        "empty_base_tiles": round(len(g.get_empty_base_tile_coordinates()) / (rows * cols), 4),
        "flat_copy_of_base_level": {"bytes": level_b, "ms": round(copy_ms, 4)},
        "base": dict(base, measure_of_flat_copy=round(base["measure_ms"] / copy_ms, 2),
                     writing_call_of_flat_copy=round(base["writing_call_ms"] / copy_ms, 2)),
        "all_levels": {"tiles": all_tiles, "writing_call_ms": round(all_ms, 4),
                       "measure_ms": round(sum(p["measure_ms"] for p in per_level), 4),
                       "write_ms": round(sum(p["write_ms"] for p in per_level), 4),
                       "tiles_per_s": round(all_tiles / all_ms * 1e3, 1),
                       "output_bytes": sum(p["output_bytes"] for p in per_level)},
        "levels": per_level,
        "pillow": pillow,
    }
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
