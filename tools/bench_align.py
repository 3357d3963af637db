#!/usr/bin/env python3
"""Times the align step's registration (tmh_register_shifts_device) on 64 pairs
of 2160 x 2560 and of one padded shape (1040 x 1392 -> lines of 2160 x 2880)
and writes one JSON document (default profiles/r10/bench_align.json):

* per kernel (reg_sums, reg_rows_fwd, reg_cols, reg_rows_inv, reg_argmax) the
  HIP-event time of the library per call, warm-up and several repetitions in
  this one process, and pairs/s of the whole call (wall, host results included);
* the bytes each pass moves, and what the box's flat copy
  (``tmh_box_probe_device`` mode 2, same process) would need for them;
* numpy's FFT correlation (float32 rfft2 / irfft2, three transforms a pair) on
  the granted cores, one pair per thread at a time -- the host comparison.

The references are synthetic sites generated on the device; target i is its
reference rolled cyclically by a known shift, so the returned shifts are
checked as well.

    python tools/bench_align.py [--pairs 64] [--out FILE]
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
from tmlibrary_amd.models.file import granted_cores  # noqa: E402

KERNELS = ("reg_sums", "reg_rows_fwd", "reg_cols", "reg_rows_inv", "reg_argmax")


def smooth_length(L):
    def smooth(n):
        for p in (2, 3, 5):
            while n % p == 0:
                n //= p
        return n == 1
    if smooth(L):
        return L
    m = 2 * L - 1
    while not smooth(m):
        m += 1
    return m


def numpy_rate(targets, refs, threads):
    from concurrent.futures import ThreadPoolExecutor

    def one(i):
        t = targets[i].astype(np.float32)
        r = refs[i].astype(np.float32)
        t -= t.mean()
        r -= r.mean()
        c = np.fft.irfft2(np.conj(np.fft.rfft2(t)) * np.fft.rfft2(r), s=t.shape)
        return int(np.argmax(c))
    n = len(targets)
    with ThreadPoolExecutor(threads) as ex:
        t0 = time.perf_counter()
        list(ex.map(one, range(n)))
        dt = time.perf_counter() - t0
    return {"pairs": n, "threads": threads, "seconds": round(dt, 3),
            "pairs_per_s": round(n / dt, 2)}


def bench_shape(L, torch, H, W, pairs, warmup, reps, copy_gbs, host_pairs, threads):
    dev = torch.device("cuda", 0)
    refs = torch.empty((pairs, H, W), dtype=torch.int16, device=dev)
    hip.check(L.tmh_synth_sites_device(C.c_void_p(refs.data_ptr()), pairs, H, W, 12345, 0, 0, 0,
                                       None))
    hip.check(L.tmh_synchronize(None))
    rng = np.random.default_rng(1)
    want_y = rng.integers(-20, 21, pairs)
    want_x = rng.integers(-20, 21, pairs)
    # T[r, c] = R[r + dy, c + dx] cyclically
    targets = torch.stack([torch.roll(refs[i], (-int(want_y[i]), -int(want_x[i])), (0, 1))
                           for i in range(pairs)])
    torch.cuda.synchronize()
    ref_of = np.arange(pairs, dtype=np.int32)
    y, x = np.zeros(pairs, np.int32), np.zeros(pairs, np.int32)
    peak = np.zeros(pairs, np.float32)
    sb = int(L.tmh_register_scratch_bytes(pairs, pairs, H, W))
    scratch = torch.empty(sb, dtype=torch.uint8, device=dev)

    def call():
        hip.check(L.tmh_register_shifts_device(
            C.c_void_p(targets.data_ptr()), pairs, C.c_void_p(refs.data_ptr()), pairs, H, W, 2,
            hip.ptr(ref_of), C.c_void_p(scratch.data_ptr()), sb, hip.ptr(y), hip.ptr(x),
            hip.ptr(peak), None))

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
    kernels = {}
    for name in KERNELS:
        ms, launches = kernel_ms(L, name)
        kernels[name] = {"ms_per_call": round(ms / reps, 4), "launches_per_call": launches // reps}
    hip.check(L.tmh_profile_enable(0))
    correct = bool(np.array_equal(y, want_y) and np.array_equal(x, want_x))

    Mh, Mw = smooth_length(H), smooth_length(W)
    z = H * Mw * 8
    moved = {"reg_sums": 2 * H * W * 2, "reg_rows_fwd": 2 * H * W * 2 + z, "reg_cols": 2 * z,
             "reg_rows_inv": z}
    for name, b in moved.items():
        k = kernels[name]
        k["bytes_per_pair"] = b
        k["flat_copy_ms_per_call"] = round(b * pairs / (copy_gbs * 1e6), 4)
        k["gb_per_s"] = round(b * pairs / (k["ms_per_call"] * 1e6), 1) if k["ms_per_call"] else None
        k["x_flat_copy"] = (round(k["ms_per_call"] / k["flat_copy_ms_per_call"], 2)
                            if k["flat_copy_ms_per_call"] else None)
    wall = float(np.median(walls))
    out = {"shape": [H, W], "line_lengths": [Mh, Mw], "pairs": pairs, "shifts_correct": correct,
           "scratch_mb": round(sb / 2 ** 20, 1), "wall_ms_median": round(wall * 1e3, 3),
           "wall_ms_min": round(min(walls) * 1e3, 3), "pairs_per_s": round(pairs / wall, 1),
           "kernel_ms_per_call": round(sum(k["ms_per_call"] for k in kernels.values()), 4),
           "kernels": kernels}
    h_t = targets[:host_pairs].cpu().numpy().view(np.uint16)
    h_r = refs[:host_pairs].cpu().numpy().view(np.uint16)
    out["numpy_rfft2_f32"] = numpy_rate(h_t, h_r, threads)
    out["x_numpy"] = round(out["pairs_per_s"] / out["numpy_rfft2_f32"]["pairs_per_s"], 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--shapes", default="2160x2560,1040x1392")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join("profiles", "r10", "bench_align.json"))
    a = ap.parse_args()
    import torch
    L = hip.lib()
    threads = max(1, min(16, granted_cores()))

    # the box's flat copy: read 2 B/px and write them, 256 MiB each way
    npx, probe_sites = 1 << 20, 128
    copy_ms = C.c_double()
    with hip.DeviceBuffer(probe_sites * npx * 2) as d_a, \
            hip.DeviceBuffer(probe_sites * npx * 2) as d_b:
        ptrs = np.array([d_a.ptr.value, d_b.ptr.value], dtype=np.uint64)
        with hip.DeviceBuffer.from_array(ptrs) as d_ptrs:
            for reps in (a.warmup, a.reps):
                hip.check(L.tmh_box_probe_device(d_ptrs, d_ptrs.at(8), 24, probe_sites, 1024, 1024,
                                                 2, reps, None, C.byref(copy_ms), None))
    copy_gbs = 2 * probe_sites * npx * 2 / (copy_ms.value * 1e6)  # bytes read + written

    doc = {"tool": "bench_align", "flat_copy_gb_per_s": round(copy_gbs, 1), "threads": threads,
           "shapes": []}
    for s in a.shapes.split(","):
        H, W = (int(v) for v in s.split("x"))
        doc["shapes"].append(bench_shape(L, torch, H, W, a.pairs, a.warmup, a.reps, copy_gbs,
                                         min(a.pairs, threads), threads))
    text = json.dumps(doc, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
