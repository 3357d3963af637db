"""CPU: the GPU inflate's decode core, built for the host, against zlib.

tmlibrary_amd/csrc/inflate_core.h is the exact code k_inflate runs per lane
(inflate_kernels.hip includes it); tests/inflate_host.cpp compiles it with g++
and runs the lanes one after another.  So every round's CPU suite checks the
decoder byte for byte against zlib -- the library behind the reference's h5py
deflate filter (tmlib/models/file.py:322-351) -- over every block kind and
the corrupt-stream statuses, without a GPU; tests/test_gpu_inflate.py runs the
same streams through the device kernel.

The hand-built streams of tests/inflate_cases.py (families A to E: format
corners zlib's encoder never emits, the match resolver's patterns, one stream
per status clause, every bit flip and truncation of four seeds, layouts) run
through two builds of the harness: the plain one and one with
-fsanitize=address,undefined, whose buffers have exactly the sizes the chunk
table states.  Expected bytes and statuses come from replaying the tokens and
from zlib, never from the decoder.
"""
import os
import subprocess
import zlib

import numpy as np
import pytest

import inflate_cases as ic
from util import REPO

HARNESS = os.path.join(REPO, "tests", "inflate_host.cpp")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("inflate") / "inflate_host")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wno-unknown-pragmas", "-o", out, HARNESS],
                   check=True, capture_output=True)
    return out


def _run(exe, tmp_path, streams, raw_lens=None):
    from tmlibrary_amd.hip import ZCHUNK_DTYPE
    n = len(streams)
    tab = np.zeros(n, ZCHUNK_DTYPE)
    off = roff = 0
    for i, (_, raw, s) in enumerate(streams):
        rl = len(raw) if raw_lens is None else raw_lens[i]
        tab[i] = (off, len(s), roff, rl, i, 0, 0, 0, 0)
        off += len(s)
        roff += rl
    p = lambda name: str(tmp_path / name)  # noqa: E731
    open(p("tab"), "wb").write(tab.tobytes())
    open(p("blob"), "wb").write(b"".join(s for _, _, s in streams))
    subprocess.run([exe, p("tab"), p("blob"), str(roff), p("out"), p("st")], check=True)
    out = open(p("out"), "rb").read()
    st = np.fromfile(p("st"), np.int32)
    return [out[t["raw_off"]:t["raw_off"] + t["raw_len"]] for t in tab], st


def test_every_block_kind(exe, tmp_path):
    from test_gpu_inflate import _streams
    streams = _streams()
    outs, st = _run(exe, tmp_path, streams)
    assert not [(s[0], int(c)) for s, c in zip(streams, st) if c]
    for (name, raw, s), got in zip(streams, outs):
        assert got == zlib.decompress(s) == raw, name


def test_random_streams(exe, tmp_path):
    rng = np.random.default_rng(2024)
    streams = []
    for i in range(200):
        kind = i % 4
        n = int(rng.integers(1, 30000))
        if kind == 0:
            raw = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        elif kind == 1:
            raw = (rng.integers(0, 40, n, dtype=np.uint16) + 900).tobytes()
        elif kind == 2:
            raw = bytes(rng.choice([0, 1, 2, 255], n).astype(np.uint8))
        else:
            raw = (np.cumsum(rng.integers(-2, 3, n)) % 5000).astype(np.uint16).tobytes()
        co = zlib.compressobj(int(rng.integers(0, 10)), zlib.DEFLATED, int(rng.integers(9, 16)),
                              int(rng.integers(1, 10)),
                              int(rng.choice([zlib.Z_DEFAULT_STRATEGY, zlib.Z_FILTERED,
                                              zlib.Z_HUFFMAN_ONLY, zlib.Z_RLE, zlib.Z_FIXED])))
        streams.append(("r%d" % i, raw, co.compress(raw) + co.flush()))
    outs, st = _run(exe, tmp_path, streams)
    assert not np.any(st)
    for (name, raw, _), got in zip(streams, outs):
        assert got == raw, name


def test_corrupt_streams(exe, tmp_path):
    raw = (np.arange(20000, dtype=np.uint16) % 1234).tobytes()
    good = zlib.compress(raw, 6)
    flipped = bytearray(good)
    flipped[len(good) // 2] ^= 0x5A
    streams = [("good", raw, good), ("truncated", raw, good[: len(good) // 2]),
               ("bad_adler", raw, good[:-1] + bytes([good[-1] ^ 1])),
               ("flipped", raw, bytes(flipped)), ("not_zlib", raw, b"\x1f\x8b" + good[2:]),
               ("good2", raw, good)]
    outs, st = _run(exe, tmp_path, streams)
    assert st[0] == 0 and st[5] == 0 and outs[0] == raw and outs[5] == raw
    assert st[1] != 0 and st[2] == 7 and st[3] != 0 and st[4] == 1
    _, st = _run(exe, tmp_path, [("s", raw, good), ("l", raw, good)],
                 [len(raw) - 10, len(raw) + 10])
    assert st[0] == 5 and st[1] == 8
    # random garbage never escapes a status (and never crashes the harness)
    rng = np.random.default_rng(3)
    junk = [("j%d" % i, b"", bytes([0x78, 0x9C]) + rng.integers(0, 256, 300, dtype=np.uint8).tobytes())
            for i in range(100)]
    _, st = _run(exe, tmp_path, junk, [4096] * 100)
    assert np.all(st != 0)


def test_junk_streams_at_raw_lengths_0_1_4096(exe, tmp_path):
    rng = np.random.default_rng(3)
    junk = [("j%d" % i, b"", bytes([0x78, 0x9C]) + rng.integers(0, 256, 300, dtype=np.uint8).tobytes())
            for i in range(100)]
    for s in junk:
        with pytest.raises(zlib.error):
            zlib.decompress(s[2])
    for raw_len in (0, 1, 4096):
        _, st = _run(exe, tmp_path, junk, [raw_len] * 100)
        assert np.all(st != 0), raw_len


# ---- the hand-built families, through a plain and a sanitized build

def build_harness(out_dir, sanitized):
    out = os.path.join(str(out_dir), "inflate_host_san" if sanitized else "inflate_host")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitized \
        else ["-O2"]
    subprocess.run(["g++", "-std=c++17", "-Wno-unknown-pragmas"] + flags + ["-o", out, HARNESS],
                   check=True, capture_output=True)
    return out


def table_of(rows):
    from tmlibrary_amd.hip import ZCHUNK_DTYPE
    tab = np.zeros(len(rows), ZCHUNK_DTYPE)
    for i, (so, sl, ro, rl, fl) in enumerate(rows):
        tab[i] = (so, sl, ro, rl, i, 0, 0, fl, 0)
    return tab


def run_batch(exe, tmp_dir, launches):
    """[(blob, rows, raw_bytes)] through one run of the harness (the output
    buffers pre-filled with the sentinel): [(raw bytes, statuses)].  The run
    must end clean: a sanitizer report is a nonzero exit."""
    jobs, outp = os.path.join(str(tmp_dir), "jobs"), os.path.join(str(tmp_dir), "out")
    with open(jobs, "wb") as f:
        for blob, rows, raw_bytes in launches:
            f.write(np.array([len(rows), len(blob), raw_bytes], np.int64).tobytes())
            f.write(table_of(rows).tobytes())
            f.write(blob)
    r = subprocess.run([exe, "--batch", jobs, outp, str(ic.SENTINEL)], capture_output=True)
    assert r.returncode == 0 and not r.stderr, r.stderr.decode(errors="replace")[-3000:]
    data, at, res = np.fromfile(outp, np.uint8), 0, []
    for blob, rows, raw_bytes in launches:
        raw = data[at:at + raw_bytes]
        at += raw_bytes
        res.append((raw, data[at:at + 4 * len(rows)].view(np.int32)))
        at += 4 * len(rows)
    assert at == len(data)
    return res


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def harness(request, tmp_path_factory):
    return build_harness(tmp_path_factory.mktemp("inflate_" + request.param),
                         request.param == "sanitized")


def _check_launches(harness, tmp_path, named):
    """named: [(name, cases, layout arguments)]"""
    lay = [ic.layout(cases, **kw) for _, cases, kw in named]
    for (name, cases, _), (_, rows, _), (raw, st) in zip(named, lay, run_batch(harness, tmp_path, lay)):
        ic.check_outputs(cases, rows, raw, st, name)


@pytest.mark.parametrize("family", ["A", "B", "C"])
def test_hand_built_family(harness, tmp_path, family):
    """A, B: exact bytes; C: the exact status of every clause (and nothing
    written past the fault).  Each of B's capacity streams also alone, so
    that the match list is sized by its own raw_len."""
    cases = ic.families()[family]
    named = [(family, cases, {})]
    named += [(c.name, [c], {}) for c in cases if c.name.startswith("cap_")]
    _check_launches(harness, tmp_path, named)


def test_incomplete_codes_rejected_as_zlib_does(harness, tmp_path):
    """zlib's inflate_table takes an incomplete code only as exactly one code
    of length 1 (for distances also none at all), and never for the
    code-length code.  These streams decode token by token to bytes with the
    right Adler-32, and zlib raises on each: TMH_Z_TABLE.  The incomplete
    codes zlib does take (family A) stay valid."""
    bad = ic.incomplete_codes()
    assert len(bad) >= 7
    for c in bad:
        with pytest.raises(zlib.error, match="invalid (literal/lengths|distances|code lengths) set|"
                                             "missing end-of-block"):
            zlib.decompress(c.stream)
    legal = [c for c in ic.families()["A"] if c.name in (
        "one_distance_code_length_1", "no_distance_code", "end_of_block_only_literal_code")]
    assert len(legal) == 3
    _check_launches(harness, tmp_path, [("incomplete", bad + legal, {})])


def test_mutants_follow_zlib(harness, tmp_path):
    """Every single-bit flip and truncation of the four seeds, none left out:
    status 0 with zlib's bytes where zlib accepts the stream at the seed's
    length, an error where it raises or gives another length; and the flips
    that leave a valid deflate stream, resealed, decode as zlib does."""
    cases = ic.families()["D"]
    n_seed_bytes = sum(len(s) for _, _, s in ic.seeds())
    assert sum("_resealed" not in c.name for c in cases) == 9 * n_seed_bytes
    assert sum("_resealed" in c.name for c in cases) > 3000
    groups = ic.split_launches(cases)
    _check_launches(harness, tmp_path, [("D%d" % i, g, {}) for i, g in enumerate(groups)])


def test_layouts(harness, tmp_path):
    """Source offsets 0..39 x output offsets x trailing bytes, launch sizes
    around the workgroup widths, the families mixed in one launch, and
    stored (filter skipped) chunks between deflated ones."""
    jobs = ic.family_e()
    assert len(jobs) == 40 * 4 * 5 + 10 + 2
    _check_launches(harness, tmp_path, jobs)
