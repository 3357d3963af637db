"""The PNG encoder's case list, shared by test_png_cpu.py (host build of
png_core.h) and test_gpu_png.py (the kernels): the smallest images where the
coder can go wrong.  Built once per process.  With P = tmh_png_piece_bytes():
no left neighbour and no upper row (1 x 1, 1 x 9, 9 x 1); a segment that ends
inside a row (97 x 253 uint16: 49,179 filtered bytes); streams that end one row
before, exactly on and one row after a piece boundary (W = 511 uint8: 512
stream bytes a row); batches, one with more pieces than the persistent grid has
workgroups; rows a multiple of 16 bytes (the filter's vector form) and not."""
import functools
import os
import subprocess

import numpy as np

from util import REPO

HARNESS = os.path.join(REPO, "tests", "png_host.cpp")


def piece_bytes():
    from tmlibrary_amd import hip
    return int(hip.load_library().tmh_png_piece_bytes())


def smooth(shape, dtype, seed):
    """A smooth 2-D field with Poisson noise: what a stained site looks like."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[:shape[0], :shape[1]]
    top = 200 if dtype == np.uint8 else 3000
    field = top * (0.3 + 0.25 * np.sin(y / 17.0) * np.cos(x / 23.0) + 0.2 * np.exp(
        -((y - shape[0] / 2.0) ** 2 + (x - shape[1] / 3.0) ** 2) / (2.0 * (max(shape) / 5.0) ** 2)))
    return np.minimum(rng.poisson(field), np.iinfo(dtype).max).astype(dtype)


@functools.lru_cache(maxsize=None)
def cases():
    """((name, images [n, H, W] uint8 / uint16), ...)"""
    rng = np.random.default_rng(2003)
    P = piece_bytes()
    out = []
    for dt, tag in ((np.uint8, "u8"), (np.uint16, "u16")):
        top = np.iinfo(dt).max
        for h, w in ((1, 1), (1, 9), (9, 1)):
            out.append(("%dx%d_%s" % (h, w, tag), rng.integers(0, top + 1, (1, h, w)).astype(dt)))
    out.append(("3x5_u8", rng.integers(0, 256, (1, 3, 5)).astype(np.uint8)))
    out.append(("zeros", np.zeros((1, 97, 253), np.uint16)))
    out.append(("constant", np.full((1, 97, 253), 0xABCD, np.uint16)))
    out.append(("random", rng.integers(0, 65536, (1, 97, 253)).astype(np.uint16)))  # the stored route
    out.append(("hramp", np.broadcast_to(np.arange(304, dtype=np.uint16) * 7, (1, 40, 304)).copy()))
    out.append(("vramp", np.broadcast_to((np.arange(60, dtype=np.uint16) * 1000)[:, None],
                                         (1, 60, 70)).copy()))
    out.append(("hramp_u8", np.broadcast_to(np.arange(300) % 256, (1, 33, 300)).astype(np.uint8)))
    out.append(("smooth", smooth((200, 500), np.uint16, 1)[None]))      # 200,400 bytes: five pieces at P = 49,152
    out.append(("smooth_v16", smooth((64, 256), np.uint16, 2)[None]))   # rows of 512 bytes: the vector form
    out.append(("smooth_u8_v16", smooth((50, 320), np.uint8, 3)[None]))
    for k, h in enumerate((P // 512 - 1, P // 512, P // 512 + 1)):
        out.append(("edge_%d" % (k - 1), smooth((h, 511), np.uint8, 10 + k)[None]))
    out.append(("batch3", np.stack([smooth((97, 253), np.uint16, 20),
                                    rng.integers(0, 65536, (97, 253)).astype(np.uint16),
                                    (smooth((97, 253), np.uint16, 21) >> 4) << 4])))
    # more pieces than k_png_pieces has workgroups (512): the grid loop runs
    out.append(("batch520", rng.integers(0, 40, (520, 8, 8)).astype(np.uint8)))
    # a plaid of smooth row and column terms: Average and Paeth rows
    y, x = np.mgrid[:48, :200]
    out.append(("plaid", ((y * y * 3 + x * 5 + (x * y) // 7) % 251).astype(np.uint8)[None]))
    return tuple(out)


def build_harness(out, sanitize=False):
    cmd = ["g++", "-O2", "-std=c++17", "-Wno-unknown-pragmas"]
    if sanitize:
        cmd += ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    subprocess.run(cmd + ["-o", out, HARNESS], check=True, capture_output=True)
    return out


def run_harness(exe, tmpdir, stacks):
    """The host core's files of the image stacks: per stack a list of ``bytes``."""
    p = lambda name: os.path.join(str(tmpdir), name)  # noqa: E731
    with open(p("cases"), "wb") as f:
        for a in stacks:
            n, h, w = a.shape
            f.write(np.array([n, h, w, a.itemsize], np.int64).tobytes())
            f.write(np.ascontiguousarray(a).tobytes())
    subprocess.run([exe, p("cases"), p("out"), p("olens")], check=True)
    blob = open(p("out"), "rb").read()
    lens = np.fromfile(p("olens"), np.int64)
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    assert offs[-1] == len(blob) and len(lens) == sum(a.shape[0] for a in stacks)
    out, i = [], 0
    for a in stacks:
        out.append([blob[offs[i + k]:offs[i + k + 1]] for k in range(a.shape[0])])
        i += a.shape[0]
    return out
