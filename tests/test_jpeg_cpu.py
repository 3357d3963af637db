"""CPU: the JPEG rules and the GPU encoder's core, against libjpeg-turbo.

tests/jpeg_literal.py restates the rules in numpy;
tests/golden/jpeg_tiles.npz holds the files Pillow's bundled libjpeg-turbo
writes for a fixed case list.  tmlibrary_amd/csrc/jpeg_core.h is the exact
per-block code k_jpeg_tiles runs (jpeg_kernels.hip includes it);
tests/jpeg_host.cpp compiles it with g++ and encodes tiles one after another.
So the CPU suite checks the encoder's arithmetic byte for byte without a GPU;
tests/test_gpu_jpeg.py runs the same cases through the device kernel.
"""
import io
import os
import subprocess

import numpy as np
import pytest

import jpeg_literal as jl
from util import REPO

HARNESS = os.path.join(REPO, "tests", "jpeg_host.cpp")
GOLDEN = os.path.join(REPO, "tests", "golden", "jpeg_tiles.npz")


@pytest.fixture(scope="module")
def goldens():
    return jl.load_goldens(GOLDEN)


@pytest.fixture(scope="module")
def random_set():
    """30 seeded tiles of random ragged shape, kind and quality, with the
    literal's bytes (computed once)."""
    rng = np.random.default_rng(95)
    kinds = ("noise", "cells", "specks", "smooth", "stripes", "ramp")
    out = []
    for i in range(30):
        h, w = (int(v) for v in rng.integers(1, 257, 2))
        if i % 5 == 0:
            h, w = min(h, 40), min(w, 40)
        q = int(rng.choice([1, 5, 10, 30, 50, 75, 90, 95, 100, int(rng.integers(1, 101))]))
        a = jl.case_array(kinds[i % len(kinds)], (h, w), seed=1000 + i)
        out.append((a, q, jl.encode(a, q)))
    return out


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("jpeg") / "jpeg_host")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-o", out,
                    HARNESS], check=True, capture_output=True)
    return out


def _run(exe, tmp_path, tiles):
    """tiles: (array, quality) -> the harness's files."""
    p = lambda name: str(tmp_path / name)  # noqa: E731
    with open(p("in"), "wb") as f:
        for a, q in tiles:
            f.write(np.array([a.shape[0], a.shape[1], q], dtype=np.int32).tobytes())
            f.write(np.ascontiguousarray(a).tobytes())
    subprocess.run([exe, p("in"), p("out"), p("sizes")], check=True)
    blob = open(p("out"), "rb").read()
    ends = np.cumsum(np.fromfile(p("sizes"), np.int64))
    assert len(ends) == len(tiles) and ends[-1] == len(blob)
    return [blob[int(e - s):int(e)] for s, e in zip(np.diff(ends, prepend=0), ends)]


def test_literal_equals_every_golden(goldens):
    assert len(goldens) == len(jl.GOLDEN_CASES) == 19
    for name, a, q, want in goldens:
        assert jl.encode(a, q) == want, name
    by = {g[0]: g for g in goldens}
    assert len(by["zeros"][3]) == 1100 and len(by["full"][3]) == 1100
    assert len(by["ragged_1x1"][3]) in (332, 333)
    stuffed = lambda b: sum(1 for i in range(jl.HEADER_BYTES, len(b) - 2) if b[i] == 255)  # noqa: E731
    assert stuffed(by["checker8_q100"][3]) == 249 and stuffed(by["stripes"][3]) == 1536


def test_goldens_are_what_the_generator_writes(goldens):
    """The stored inputs are GOLDEN_CASES' arrays (the GPU tests rebuild
    nothing, but a changed case list must regenerate the file)."""
    for (name, a, q, _), (n2, kind, shape, q2) in zip(goldens, jl.GOLDEN_CASES):
        assert name == n2 and q == q2 and np.array_equal(a, jl.case_array(kind, shape)), name


def test_literal_equals_pillow_on_random_tiles(random_set):
    Image = pytest.importorskip("PIL.Image")
    for a, q, got in random_set:
        buf = io.BytesIO()
        Image.fromarray(a, "L").save(buf, "JPEG", quality=q)
        assert got == buf.getvalue(), (a.shape, q)


def test_core_equals_goldens_and_literal(exe, tmp_path, goldens, random_set):
    """The kernel's per-block code, built for the host."""
    got = _run(exe, tmp_path, [(a, q) for _, a, q, _ in goldens])
    for (name, _, _, want), g in zip(goldens, got):
        assert g == want, name
    got = _run(exe, tmp_path, [(a, q) for a, q, _ in random_set])
    for (a, q, want), g in zip(random_set, got):
        assert g == want, (a.shape, q)
    # the quality clamp of jpeg_set_quality
    a = jl.case_array("cells", (40, 24))
    lo, lo2, hi, hi2 = _run(exe, tmp_path, [(a, 0), (a, -5), (a, 101), (a, 1000)])
    assert lo == lo2 == jl.encode(a, 1) and hi == hi2 == jl.encode(a, 100)


def test_core_division_by_multiplication(exe):
    """jpeg_quantise's reciprocal multiply equals the division for every
    quantiser 1..255 and every 16-bit coefficient."""
    assert subprocess.run([exe, "--division"]).returncode == 0


def test_header_constants():
    h = jl.header(37, 101, 95)
    assert len(h) == jl.HEADER_BYTES == 328
    # segment order and lengths: SOI, APP0 (18), DQT (69), SOF0 (13), DHT (33), DHT (183), SOS (10)
    at, seen = 2, []
    assert h[:2] == b"\xFF\xD8"
    while at < len(h):
        assert h[at] == 0xFF
        n = (h[at + 2] << 8 | h[at + 3]) + 2
        seen.append((h[at + 1], n))
        at += n
    assert at == 328
    assert seen == [(0xE0, 18), (0xDB, 69), (0xC0, 13), (0xC4, 33), (0xC4, 183), (0xDA, 10)]
    assert h[6:11] == b"JFIF\0" and h[11:20] == bytes([1, 1, 0, 0, 1, 0, 1, 0, 0])
    assert h[94:98] == bytes([0, 37, 0, 101])
    assert bytes(h[25:89]) == bytes(int(jl.quant_table(95)[i]) for i in jl.ZIGZAG)
    assert jl.quant_table(100).tolist() == [1] * 64 and jl.quant_table(0).tolist() == \
        jl.quant_table(1).tolist() and jl.quant_table(1).max() == 255
    other = jl.header(256, 256, 50)
    diff = [i for i in range(328) if other[i] != h[i]]
    assert set(diff) <= set(range(25, 89)) | set(range(94, 98))
