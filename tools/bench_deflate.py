#!/usr/bin/env python3
"""Site-image output path on the GPU box: GPU deflate vs host zlib.

For the standard and the bright synthetic layouts, B sites of 2160 x 2560
uint16 (D distinct ones cycled) in h5py's default 135 x 160 chunks:
  kernels:  tmh_gather_chunks_device, tmh_deflate_device (deflate, compaction), per block
  encode:   sites/s of gather + deflate + compaction, device sites in, packed streams out
  copy:     a flat device copy of the same raw bytes (what the box moves at best)
  files:    write_channel_images_device (encode + D2H + H5Dwrite_chunk), sites/s
  host:     zlib levels 1 and 4 on the granted cores (chunks in parallel), sites/s
  size:     compressed bytes against zlib levels 1 and 4 on the distinct sites,
            and on the structured set of tests/deflate_cases.py
and the round trip through tmh_inflate_device is checked.  One JSON document.
    python tools/bench_deflate.py [--block 128] [--distinct 8] [--reps 3] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import shutil
import sys
import tempfile
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import numpy as np  # noqa: E402


def chunk_list(sites, cr, cc):
    from deflate_cases import chunkify
    return [c for s in sites for c in chunkify(s, cr, cc)]


def host_zlib(chunks, level, pool):
    t = time.perf_counter()
    sizes = list(pool.map(lambda c: len(zlib.compress(c, level)), chunks))
    return sum(sizes), time.perf_counter() - t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--block", type=int, default=128)
    ap.add_argument("--distinct", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--width", type=int, default=2560)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    import deflate_cases as dc
    from tmlibrary_amd import hip, synth
    from tmlibrary_amd.models.device_encode import DeviceChunkEncoder, write_channel_images_device
    from tmlibrary_amd.models.file import granted_cores, h5py_chunk_shape, read_channel_image
    L = hip.lib()
    H, W, B, D = a.height, a.width, a.block, a.distinct
    cr, cc = h5py_chunk_shape((H, W), 2)
    cores = granted_cores()
    pool = ThreadPoolExecutor(cores)
    dev = torch.device("cuda", 0)
    enc = DeviceChunkEncoder(device=dev, slots=1)
    res = {"sites": B, "distinct": D, "height": H, "width": W, "chunk": [cr, cc],
           "host_threads": cores, "layouts": {}}

    def prof(names):
        out = {}
        for name in names:
            ms, k = C.c_double(), C.c_int64()
            hip.check(L.tmh_profile_read(name.encode(), C.byref(ms), C.byref(k)))
            if k.value:
                out[name] = round(ms.value / k.value, 3)
        return out

    for lname, dist in (("standard", synth.STANDARD), ("bright", synth.BRIGHT)):
        host = np.stack([synth.synth_exact_host(H, W, 12345, 0, i, dist) for i in range(D)])
        sites = torch.from_numpy(host.view(np.int16)).to(dev)[torch.arange(B, device=dev) % D]
        sites = sites.contiguous()
        torch.cuda.synchronize()
        r = {}
        blob, table, geom = enc.deflate(sites)  # warm-up: buffers sized
        L.tmh_profile_enable(1)
        L.tmh_profile_reset()
        tt = []
        for _ in range(a.reps):
            torch.cuda.synchronize()
            t = time.perf_counter()
            blob, table, geom = enc.deflate(sites)
            tt.append(time.perf_counter() - t)
        r["kernel_ms_per_block"] = prof(("gather_chunks", "deflate", "deflate_compact"))
        L.tmh_profile_enable(0)
        kern = sum(r["kernel_ms_per_block"].values())
        r["kernels_sites_per_s"] = round(B / (kern * 1e-3), 1) if kern else None
        r["kernels_raw_GBs"] = round(B * H * W * 2 / (kern * 1e-3) / 1e9, 2) if kern else None
        r["encode_call_sites_per_s"] = round(B / min(tt), 1)  # with the D2H of table and streams
        r["compressed_bytes_per_site"] = round(len(blob) / B, 1)
        r["size_over_raw"] = round(len(blob) / (B * H * W * 2), 4)
        # the box's flat copy of the same bytes
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
        # files
        d = tempfile.mkdtemp(prefix="tmh_deflate_")
        paths = [os.path.join(d, "channel_image_file_%d.h5" % i) for i in range(B)]
        t = time.perf_counter()
        write_channel_images_device(paths, sites)
        r["files_sites_per_s"] = round(B / (time.perf_counter() - t), 1)
        ok = all(np.array_equal(read_channel_image(paths[i]), host[i % D]) for i in (0, D - 1, B - 1))
        shutil.rmtree(d, ignore_errors=True)
        # size and host rate on the distinct sites
        chunks = chunk_list(host, cr, cc)
        n1, t1 = host_zlib(chunks, 1, pool)
        n4, t4 = host_zlib(chunks, 4, pool)
        ours = int(table["src_len"][:len(chunks)].sum())  # the first D sites are the distinct ones
        r["bytes_distinct"] = {"ours": ours, "zlib1": n1, "zlib4": n4}
        r["ratio_to_zlib1"] = round(ours / n1, 4)
        r["ratio_to_zlib4"] = round(ours / n4, 4)
        r["host_zlib1_sites_per_s"] = round(D / t1, 1)
        r["host_zlib4_sites_per_s"] = round(D / t4, 1)
        for k in (0, len(chunks) // 2, len(chunks) - 1):  # streams decode to the chunks
            e = table[k]
            ok = ok and zlib.decompress(blob[e["src_off"]:e["src_off"] + e["src_len"]].tobytes()) == chunks[k]
        r["round_trip_ok"] = bool(ok)
        res["layouts"][lname] = r
        print(json.dumps({lname: r}), file=sys.stderr, flush=True)
        del sites
    # structured content (tests/deflate_cases.py), image by image through the encoder
    chunks = list(dc.structured_chunks())
    ours, ok = 0, True
    for img in dc.structured_images():
        blob, table, _ = enc.deflate(img, chunks=(cr, cc))
        ours += len(blob)
        for e, c in zip(table, dc.chunkify(img, cr, cc)):
            ok = ok and zlib.decompress(blob[e["src_off"]:e["src_off"] + e["src_len"]].tobytes()) == c
    n1, _ = host_zlib(chunks, 1, pool)
    n4, _ = host_zlib(chunks, 4, pool)
    res["structured"] = {"chunks": len(chunks), "ours": ours, "zlib1": n1, "zlib4": n4,
                         "ratio_to_zlib1": round(ours / n1, 4), "ratio_to_zlib4": round(ours / n4, 4),
                         "round_trip_ok": bool(ok)}
    text = json.dumps(res, indent=1, sort_keys=True)
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
