"""CPU: the JPEG decoding rules and the GPU decoder's core, against libjpeg-turbo.

tests/jpeg_decode_literal.py restates the rules in
numpy; tests/golden/jpeg_decoded.npz holds what Pillow's bundled libjpeg-turbo
decodes from the files of jpeg_tiles.npz and from ten more tiles.
tmlibrary_amd/csrc/jpeg_core.h is the exact per-file and per-block code
k_jpeg_decode_tiles and k_jpeg_roundtrip run; tests/jpeg_decode_host.cpp
compiles it with g++.  So the CPU suite checks the decoder's arithmetic and
its handling of bad files without a GPU; tests/test_gpu_jpeg_decode.py runs
the same cases through the device kernels.
"""
import io
import os
import subprocess

import numpy as np
import pytest

import jpeg_decode_literal as jd
import jpeg_literal as jl
import pyramid_literal as lit
from util import REPO

HARNESS = os.path.join(REPO, "tests", "jpeg_decode_host.cpp")
GOLDEN = os.path.join(REPO, "tests", "golden", "jpeg_decoded.npz")
FLAGS = ["-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas"]


@pytest.fixture(scope="module")
def goldens():
    return jd.load_goldens(GOLDEN)


@pytest.fixture(scope="module")
def random_set():
    """30 seeded tiles of random ragged shape, kind and quality, with the
    literal's file and round trip (computed once)."""
    rng = np.random.default_rng(14)
    kinds = ("noise", "cells", "specks", "smooth", "stripes", "ramp", "checker1", "impulses")
    out = []
    for i in range(30):
        h, w = (int(v) for v in rng.integers(1, 257, 2))
        if i % 3:
            h, w = min(h, 48), min(w, 48)
        q = int(rng.choice([1, 5, 10, 30, 50, 75, 90, 95, 100, int(rng.integers(1, 101))]))
        a = jl.case_array(kinds[i % len(kinds)], (h, w), seed=1400 + i)
        out.append((a, q, jl.encode(a, q), jd.roundtrip(a, q)))
    return out


@pytest.fixture(scope="module")
def cases(goldens):
    z = np.load(GOLDEN)
    base = [g for g in goldens if g[0] == "extra7"][0]
    bad = jd.status_cases(base[3], {k[4:]: z[k] for k in z.files if k.startswith("bad_")})
    return base, bad, jd.good_variants(base[3])


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("jpegd") / "jpeg_decode_host")
    subprocess.run(["g++", "-O2"] + FLAGS + ["-o", out, HARNESS], check=True, capture_output=True)
    return out


def _decode(exe, tmp_path, files):
    """files -> [(array or None, status)] of the harness."""
    p = lambda name: str(tmp_path / name)  # noqa: E731
    offsets = np.concatenate([[0], np.cumsum([len(f) for f in files])]).astype(np.int64)
    with open(p("in"), "wb") as f:
        f.write(np.array([len(files)], dtype=np.int64).tobytes() + offsets.tobytes() + b"".join(files))
    subprocess.run([exe, "decode", p("in"), p("out")], check=True)
    raw, at, out = open(p("out"), "rb").read(), 0, []
    for _ in files:
        status, h, w = np.frombuffer(raw, np.int32, 3, at)
        at += 12
        assert (status == 0) == (h > 0 and w > 0)
        out.append((np.frombuffer(raw, np.uint8, h * w, at).reshape(h, w) if status == 0 else None,
                    int(status)))
        at += h * w
    assert at == len(raw)
    return out


def _roundtrip(exe, tmp_path, tiles):
    p = lambda name: str(tmp_path / name)  # noqa: E731
    with open(p("rin"), "wb") as f:
        for a, q in tiles:
            f.write(np.array([a.shape[0], a.shape[1], q], dtype=np.int32).tobytes())
            f.write(np.ascontiguousarray(a).tobytes())
    subprocess.run([exe, "roundtrip", p("rin"), p("rout")], check=True)
    raw, at, out = open(p("rout"), "rb").read(), 0, []
    for a, _ in tiles:
        out.append(np.frombuffer(raw, np.uint8, a.size, at).reshape(a.shape))
        at += a.size
    assert at == len(raw)
    return out


def test_literal_equals_every_golden(goldens):
    assert len(goldens) == 19 + 10
    assert sorted({g[2] for g in goldens[19:]}) == [1, 30, 50, 75, 90, 95, 100]
    for name, a, q, data, want in goldens:
        assert want.shape == a.shape and want.dtype == np.uint8, name
        got, status = jd.decode(data)
        assert status == 0 and np.array_equal(got, want), name
        assert np.array_equal(jd.roundtrip(a, q), want), name
    # the round trip is lossy where it should be, and nowhere else
    by = {g[0]: g for g in goldens}
    assert np.array_equal(by["zeros"][4], by["zeros"][1])
    assert not np.array_equal(by["noise"][4], by["noise"][1])


def test_literal_equals_pillow_on_random_tiles(random_set):
    Image = pytest.importorskip("PIL.Image")
    for a, q, data, rt in random_set:
        want = np.array(Image.open(io.BytesIO(data)))
        assert np.array_equal(rt, want), (a.shape, q)
        got, status = jd.decode(data)
        assert status == 0 and np.array_equal(got, want), (a.shape, q)


def test_decode_of_encode_is_the_roundtrip(random_set):
    for a, q, data, rt in random_set:
        got, status = jd.decode(data)
        assert status == 0 and np.array_equal(got, rt), (a.shape, q)


def test_core_equals_goldens_and_literal(exe, tmp_path, goldens, random_set):
    """The kernels' per-file and per-block code, built for the host."""
    got = _decode(exe, tmp_path, [g[3] for g in goldens])
    for (name, _, _, _, want), (g, status) in zip(goldens, got):
        assert status == 0 and np.array_equal(g, want), name
    got = _roundtrip(exe, tmp_path, [(g[1], g[2]) for g in goldens])
    for (name, _, _, _, want), g in zip(goldens, got):
        assert np.array_equal(g, want), name
    got = _decode(exe, tmp_path, [r[2] for r in random_set])
    rts = _roundtrip(exe, tmp_path, [(r[0], r[1]) for r in random_set])
    for (a, q, _, want), (g, status), rt in zip(random_set, got, rts):
        assert status == 0 and np.array_equal(g, want), (a.shape, q)
        assert np.array_equal(rt, want), (a.shape, q)


def test_variants_that_must_decode(exe, tmp_path, cases):
    base, _, good = cases
    got = _decode(exe, tmp_path, [f for _, f in good])
    for (name, f), (g, status) in zip(good, got):
        lit_g, lit_status = jd.decode(f)
        assert lit_status == 0 and np.array_equal(lit_g, base[4]), name
        assert status == 0 and np.array_equal(g, base[4]), name


def test_status_cases(exe, tmp_path, cases):
    """Truncated, unsupported and damaged files: the literal and the harness
    give the status the rules name, and good files among them still decode."""
    base, bad, _ = cases
    assert sum(1 for name, _, _ in bad if name.startswith("cut_")) == 12
    files = [base[3]] + [f for _, f, _ in bad] + [base[3]]
    got = _decode(exe, tmp_path, files)
    for g in (got[0], got[-1]):
        assert g[1] == 0 and np.array_equal(g[0], base[4])
    for (name, f, want), (g, status) in zip(bad, got[1:-1]):
        assert jd.decode(f) == (None, want), name
        assert status == want and g is None, name


def test_status_cases_under_sanitizers(tmp_path, cases):
    """The stand-alone harness built with -fsanitize=address,undefined: every
    file sits in a heap block of its exact size, so a read past it, an index
    past a table or an overflowing shift ends the run."""
    exe = str(tmp_path / "jpeg_decode_host_san")
    r = subprocess.run(["g++", "-O1", "-g", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all"] + FLAGS + ["-o", exe, HARNESS],
                       capture_output=True, text=True)
    if r.returncode != 0 and ("asan" in r.stderr or "ubsan" in r.stderr or "sanitize" in r.stderr):
        pytest.skip("g++ here lacks the sanitizer runtimes: " + r.stderr.strip().splitlines()[-1])
    assert r.returncode == 0, r.stderr
    base, bad, good = cases
    rng = np.random.default_rng(2)
    damaged = []
    for i in range(40):  # seeded damage anywhere in the file: any status, no bad access
        f = bytearray(base[3])
        for at in rng.integers(2, len(f), 1 + i % 4):
            f[at] = int(rng.integers(0, 256))
        damaged.append(bytes(f))
    files = [base[3]] + [f for _, f, _ in bad] + [f for _, f in good] + damaged
    got = _decode(exe, tmp_path, files)
    assert [s for _, s in got[1:1 + len(bad)]] == [w for _, _, w in bad]
    for f, (g, status) in zip(damaged, got[-len(damaged):]):
        lit_g, lit_status = jd.decode(f)
        assert status == lit_status and (g is None or np.array_equal(g, lit_g))
    a, q = jl.case_array("noise", (37, 101)), 95
    assert np.array_equal(_roundtrip(exe, tmp_path, [(a, q)])[0], jd.roundtrip(a, q))


# ---- the stored pyramid ------------------------------------------------------------------

def test_stored_pyramid_differs_from_direct_halving():
    g = lit.make_layer("one_well")
    sites = lit.random_sites(g)
    stored = jd.stored_pyramid_literal(g, sites, 95)
    direct = jd.stored_pyramid_literal(g, sites, None)
    z = g.depth - 1
    assert all(np.array_equal(stored[z][0][k], direct[z][0][k]) for k in direct[z][0])
    z = g.depth - 2
    assert stored[z][1:] == direct[z][1:]
    differs = [not np.array_equal(stored[z][0][k], direct[z][0][k]) for k in direct[z][0]]
    assert all(differs)
    d = np.abs(stored[z][0][(0, 0)].astype(int) - direct[z][0][(0, 0)])
    assert 0 < d.max() <= 8      # a few DN, the size the issue measured
