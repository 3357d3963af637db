#!/usr/bin/env python3
"""PNG export on the GPU box: tmh_png_encode_device vs Pillow on the host.

For B sites of 2160 x 2560 (D distinct ones cycled) -- uint16 of the standard
(stained-well) and the bright synthetic layouts, and uint8 (standard >> 4):
  kernels:  png_filter, png_pieces, png_pack per block, and sites/s of the three
  copy:     a flat device copy of the same raw bytes (what the box moves at best)
  deflate:  tmh_gather_chunks_device + tmh_deflate_device on the same sites, and
            the ratio of the PNG kernels' time to it
  host:     Pillow save(format="PNG", compress_level=1) on the granted cores
  size:     file bytes against Pillow at levels 1 and 6 on the distinct sites
  pieces:   with --segs4-lib (a library built with -DTMH_PNG_PIECE_SEGS=4:
            EXTRA_CXXFLAGS=-DTMH_PNG_PIECE_SEGS=4 tools/build_variant.sh NAME .)
            the same kernels and sizes at four segments a piece, in a child process
and the first and last files are decoded with Pillow.  One JSON document.
    python tools/bench_png.py [--block 128] [--distinct 8] [--reps 3] [--out FILE]
"""
import argparse
import ctypes as C
import io
import json
import os
import subprocess
import sys
import time
from concurrent.futures import ThreadPoolExecutor

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402

KERNELS = ("png_filter", "png_pieces", "png_pack")


def pillow_png(site, level):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(site).save(b, format="PNG", compress_level=level)
    return b.getbuffer().nbytes


def layouts(H, W, D):
    from tmlibrary_amd import synth
    std = np.stack([synth.synth_exact_host(H, W, 12345, 0, i, synth.STANDARD) for i in range(D)])
    yield "u16_standard", std
    yield "u16_bright", np.stack([synth.synth_exact_host(H, W, 12345, 0, i, synth.BRIGHT)
                                  for i in range(D)])
    yield "u8_standard", (std >> 4).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--block", type=int, default=128)
    ap.add_argument("--distinct", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--width", type=int, default=2560)
    ap.add_argument("--segs4-lib", default=None)
    ap.add_argument("--kernels-only", action="store_true", help="the child's run: no host comparisons")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from PIL import Image

    from tmlibrary_amd import hip
    from tmlibrary_amd.models.device_encode import DeviceChunkEncoder
    from tmlibrary_amd.models.file import granted_cores
    L = hip.lib()
    H, W, B, D = a.height, a.width, a.block, a.distinct
    cores = granted_cores()
    pool = ThreadPoolExecutor(cores)
    dev = torch.device("cuda", 0)
    res = {"sites": B, "distinct": D, "height": H, "width": W, "host_threads": cores,
           "piece_bytes": int(L.tmh_png_piece_bytes()), "layouts": {}}

    def prof(names):
        out = {}
        for name in names:
            ms, k = C.c_double(), C.c_int64()
            hip.check(L.tmh_profile_read(name.encode(), C.byref(ms), C.byref(k)))
            if k.value:
                out[name] = round(ms.value / k.value, 3)
        return out

    for lname, host in layouts(H, W, D):
        es = host.itemsize
        sites = torch.from_numpy(host.view(np.int16 if es == 2 else np.uint8)).to(dev)
        sites = sites[torch.arange(B, device=dev) % D].contiguous()
        torch.cuda.synchronize()
        r = {}
        dst_bytes = B * int(L.tmh_png_bound(H, W, es))
        scr_bytes = int(L.tmh_png_scratch_bytes(B, H, W, es))
        with hip.DeviceBuffer(dst_bytes) as d_dst, hip.DeviceBuffer(scr_bytes) as d_scr, \
                hip.DeviceBuffer(8 * (B + 1)) as d_off:
            def run():
                hip.check(L.tmh_png_encode_device(C.c_void_p(sites.data_ptr()), B, H, W, es, d_dst,
                                                  dst_bytes, d_off, d_scr, scr_bytes, None))
                hip.check(L.tmh_synchronize(None))
            run()  # warm-up
            L.tmh_profile_enable(1)
            L.tmh_profile_reset()
            tt = []
            for _ in range(a.reps):
                t = time.perf_counter()
                run()
                tt.append(time.perf_counter() - t)
            r["kernel_ms_per_block"] = prof(KERNELS)
            L.tmh_profile_enable(0)
            offsets = d_off.get((B + 1,), np.int64)
            ok = True
            for i in (0, B - 1):
                f = d_dst.get((int(offsets[i + 1] - offsets[i]),), np.uint8, offset=int(offsets[i]))
                ok = ok and np.array_equal(np.array(Image.open(io.BytesIO(f.tobytes()))), host[i % D])
        kern = sum(r["kernel_ms_per_block"].values())
        r["kernels_sites_per_s"] = round(B / (kern * 1e-3), 1)
        r["kernels_raw_GBs"] = round(B * H * W * es / (kern * 1e-3) / 1e9, 2)
        r["call_sites_per_s"] = round(B / min(tt), 1)
        r["bytes_distinct"] = {"ours": int(offsets[D])}
        r["size_over_raw"] = round(int(offsets[D]) / (D * H * W * es), 4)
        r["decodes_ok"] = bool(ok)
        if not a.kernels_only:
            dst = torch.empty_like(sites)
            dst.copy_(sites)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(5):
                dst.copy_(sites)
            e1.record()
            torch.cuda.synchronize()
            r["flat_copy_ms_per_block"] = round(e0.elapsed_time(e1) / 5, 3)
            del dst
            # the deflate path on the same sites
            enc = DeviceChunkEncoder(device=dev, slots=1)
            enc.deflate(sites)
            L.tmh_profile_enable(1)
            L.tmh_profile_reset()
            for _ in range(a.reps):
                enc.deflate(sites)
            dk = prof(("gather_chunks", "deflate", "deflate_compact"))
            L.tmh_profile_enable(0)
            del enc
            r["deflate_kernel_ms_per_block"] = dk
            r["deflate_kernels_sites_per_s"] = round(B / (sum(dk.values()) * 1e-3), 1)
            r["png_over_deflate_time"] = round(kern / sum(dk.values()), 3)
            # Pillow on the granted cores
            t = time.perf_counter()
            n1 = sum(pool.map(lambda s: pillow_png(s, 1), host))
            r["host_pillow1_sites_per_s"] = round(D / (time.perf_counter() - t), 1)
            n6 = sum(pool.map(lambda s: pillow_png(s, 6), host))
            r["bytes_distinct"].update({"pillow1": n1, "pillow6": n6})
            r["ratio_to_pillow1"] = round(int(offsets[D]) / n1, 4)
            r["ratio_to_pillow6"] = round(int(offsets[D]) / n6, 4)
        res["layouts"][lname] = r
        print(json.dumps({lname: r}), file=sys.stderr, flush=True)
        del sites
        torch.cuda.empty_cache()
    if a.segs4_lib:
        env = dict(os.environ, TMH_LIB=os.path.abspath(a.segs4_lib))
        cmd = [sys.executable, os.path.abspath(__file__), "--kernels-only", "--block", str(B),
               "--distinct", str(D), "--reps", str(a.reps), "--height", str(H), "--width", str(W)]
        child = subprocess.run(cmd, env=env, check=True, capture_output=True, text=True)
        res["piece_segs_4"] = json.loads(child.stdout)
    text = json.dumps(res, indent=1, sort_keys=True)
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
