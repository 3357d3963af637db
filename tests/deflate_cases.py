"""The deflate encoder's case list, shared by test_deflate_cpu.py (host build
of deflate_core.h) and test_gpu_deflate.py (the kernel): the smallest inputs
where the coder can go wrong.  Built once per process."""
import functools
import os
import subprocess

import numpy as np

from util import GOLDEN, REPO

HARNESS = os.path.join(REPO, "tests", "deflate_host.cpp")


def bound(n):
    """tmh_deflate_bound"""
    return n + 5 * ((max(n, 1) + 65534) // 65535) + 6


def chunkify(img, rows=135, cols=160):
    """HDF5's chunks of a 2-D array: row-major, edge chunks zero padded."""
    h, w = img.shape
    out = []
    for r0 in range(0, h, rows):
        for c0 in range(0, w, cols):
            c = np.zeros((rows, cols), img.dtype)
            part = img[r0:r0 + rows, c0:c0 + cols]
            c[:part.shape[0], :part.shape[1]] = part
            out.append(c.tobytes())
    return out


@functools.lru_cache(maxsize=None)
def synth_chunks(distribution):
    from tmlibrary_amd import synth
    dist = {"standard": synth.STANDARD, "bright": synth.BRIGHT}[distribution]
    return tuple(chunkify(synth.synth_exact_host(540, 640, distribution=dist)))


@functools.lru_cache(maxsize=None)
def cases():
    """[(name, bytes)]"""
    rng = np.random.default_rng(1951)
    rnd = lambda n: rng.integers(0, 256, n, dtype=np.uint8).tobytes()  # noqa: E731
    text = (np.cumsum(rng.integers(-2, 3, 400)) % 7 + 60).astype(np.uint8).tobytes()
    out = [("len%d" % n, text[:n]) for n in (0, 1, 2, 3, 257, 258, 259)]
    out += [("random%d" % n, rnd(n)) for n in (65535, 65536, 131071)]
    # 22 segments of random bytes: over the bound until rewritten as 65,535-byte stored blocks
    out.append(("random1m", rnd(1 << 20)))
    out.append(("zeros", bytes(43200)))
    out.append(("ones", b"\xff" * 43200))
    out.append(("odd_byte", b"\x07" * 21601 + b"\x08" + b"\x07" * 21598))
    out.append(("rows", rnd(320) * 135))
    half = rnd(21600)
    out.append(("halves", half + half))
    out.append(("dist32768", (rnd(32768) * 3)[:70000]))
    out.append(("dist32769", (rnd(32769) * 3)[:70000]))
    palette = rng.choice(65536, 40, replace=False).astype(np.uint16)
    out.append(("palette", palette[rng.integers(0, 40, 21600)].tobytes()))
    for d in ("standard", "bright"):
        out += [("synth_%s_%d" % (d, i), c) for i, c in enumerate(synth_chunks(d))]
    out.append(("every_byte", rng.permutation(256).astype(np.uint8).tobytes()))
    fib = [1, 1]
    while len(fib) < 22:
        fib.append(fib[-1] + fib[-2])
    weights = np.repeat(np.arange(22, dtype=np.uint8) * 11 + 3, fib)  # 46,367 bytes: depth 21 without a limit
    out.append(("fibonacci", rng.permutation(weights).tobytes()))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def structured_images():
    """Content with structure: cells and specks (tests/golden/jpeg_tiles.npz)
    widened to uint16, and a 2160 x 2560 synth site with a 25% zero border."""
    from tmlibrary_amd import synth
    with np.load(os.path.join(GOLDEN, "jpeg_tiles.npz"), allow_pickle=False) as z:
        out = [z[k].astype(np.uint16) for k in ("in_cells", "in_specks")]
    site = synth.synth_exact_host(2160, 2560).copy()
    by, bx = 2160 // 8, 2560 // 8  # a border of an eighth per side: a quarter of each axis
    site[:by], site[-by:], site[:, :bx], site[:, -bx:] = 0, 0, 0, 0
    return tuple(out + [site])


@functools.lru_cache(maxsize=None)
def structured_chunks():
    """structured_images() cut into 135 x 160 chunks."""
    return tuple(c for img in structured_images() for c in chunkify(img))


def build_harness(out, sanitize=False):
    cmd = ["g++", "-O2", "-std=c++17", "-Wno-unknown-pragmas"]
    if sanitize:
        cmd += ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    subprocess.run(cmd + ["-o", out, HARNESS], check=True, capture_output=True)
    return out


def run_harness(exe, tmpdir, raws):
    """The host core's streams of the byte strings `raws`."""
    p = lambda name: os.path.join(str(tmpdir), name)  # noqa: E731
    with open(p("raw"), "wb") as f:
        f.write(b"".join(raws))
    np.array([len(r) for r in raws], np.int64).tofile(p("lens"))
    subprocess.run([exe, p("raw"), p("lens"), p("out"), p("olens")], check=True)
    blob = open(p("out"), "rb").read()
    lens = np.fromfile(p("olens"), np.int64)
    offs = np.concatenate([[0], np.cumsum(lens)])
    assert offs[-1] == len(blob)
    return [blob[offs[i]:offs[i + 1]] for i in range(len(raws))]
