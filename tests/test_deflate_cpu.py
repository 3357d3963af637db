"""CPU: the GPU deflate's encode core, built for the host, against zlib.

tmlibrary_amd/csrc/deflate_core.h is the exact code k_deflate_chunks runs per
workgroup (deflate_kernels.hip includes it); tests/deflate_host.cpp compiles
it with g++ as a workgroup of one thread.  Every stream of the case list
(tests/deflate_cases.py) must decode with zlib -- the library behind the
reference's h5py deflate filter (tmlib/models/file.py:322-363) -- and with the
repository's own inflate core; the size conditions are those of DESIGN §18.
tests/test_gpu_deflate.py checks that the kernel emits the same bytes.
"""
import ctypes as C
import os
import subprocess
import zlib

import numpy as np
import pytest

import deflate_cases as dc
from util import REPO


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return dc.build_harness(str(tmp_path_factory.mktemp("deflate") / "deflate_host"))


@pytest.fixture(scope="module")
def streams(exe, tmp_path_factory):
    cs = dc.cases()
    out = dc.run_harness(exe, tmp_path_factory.mktemp("deflate_run"), [r for _, r in cs])
    return {name: (raw, s) for (name, raw), s in zip(cs, out)}


def test_round_trip_zlib(streams):
    for name, (raw, s) in streams.items():
        d = zlib.decompressobj()
        assert d.decompress(s) == raw, name
        assert d.eof and d.unused_data == b"", name
        assert s[0] == 0x78 and ((s[0] << 8) | s[1]) % 31 == 0 and not s[1] & 0x20, name
        assert int.from_bytes(s[-4:], "big") == zlib.adler32(raw), name


def test_round_trip_own_inflate(streams, tmp_path):
    """tests/inflate_host.cpp (the GPU reader's decode core) takes every stream."""
    from tmlibrary_amd.hip import ZCHUNK_DTYPE
    inf = str(tmp_path / "inflate_host")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wno-unknown-pragmas", "-o", inf,
                    os.path.join(REPO, "tests", "inflate_host.cpp")], check=True, capture_output=True)
    items = list(streams.items())
    tab = np.zeros(len(items), ZCHUNK_DTYPE)
    off = roff = 0
    for i, (_, (raw, s)) in enumerate(items):
        tab[i] = (off, len(s), roff, len(raw), i, 0, 0, 0, 0)
        off += len(s)
        roff += len(raw)
    p = lambda n: str(tmp_path / n)  # noqa: E731
    open(p("tab"), "wb").write(tab.tobytes())
    open(p("blob"), "wb").write(b"".join(s for _, (_, s) in items))
    subprocess.run([inf, p("tab"), p("blob"), str(roff), p("out"), p("st")], check=True)
    st = np.fromfile(p("st"), np.int32)
    assert not [(items[i][0], int(c)) for i, c in enumerate(st) if c]
    assert open(p("out"), "rb").read() == b"".join(raw for _, (raw, _) in items)


def test_sanitizers(streams, tmp_path):
    """The same stand-alone program under ASan + UBSan, once over the case list:
    a clean exit, and the bytes of the plain build."""
    san = dc.build_harness(str(tmp_path / "deflate_host_san"), sanitize=True)
    out = dc.run_harness(san, tmp_path, [raw for raw, _ in streams.values()])
    assert out == [s for _, s in streams.values()]


def test_size_conditions(streams):
    for name, (raw, s) in streams.items():
        assert len(s) <= dc.bound(len(raw)), name
    for name in ("zeros", "ones", "odd_byte"):
        assert len(streams[name][1]) <= 512, name
    assert len(streams["rows"][1]) <= 2048
    assert len(streams["halves"][1]) <= 21600 + 2048
    # random bytes whose only repeats are out of the window: nothing to gain
    raw, s = streams["dist32769"]
    assert len(s) >= len(raw)
    for d in ("standard", "bright"):
        ours = sum(len(streams["synth_%s_%d" % (d, i)][1]) for i in range(16))
        level4 = sum(len(zlib.compress(c, 4)) for c in dc.synth_chunks(d))
        print("synth %s: ours %d, zlib level 4 %d (%.4f)" % (d, ours, level4, ours / level4))
        assert ours <= level4, d


def test_structured_content_against_level1(exe, tmp_path):
    chunks = dc.structured_chunks()
    out = dc.run_harness(exe, tmp_path, list(chunks))
    for c, s in zip(chunks, out):
        assert zlib.decompress(s) == c
    ours = sum(map(len, out))
    level1 = sum(len(zlib.compress(c, 1)) for c in chunks)
    level4 = sum(len(zlib.compress(c, 4)) for c in chunks)
    print("structured: ours %d, zlib level 1 %d (%.4f), level 4 %d (%.4f)"
          % (ours, level1, ours / level1, level4, ours / level4))
    assert ours <= level1


def test_bound_and_exports():
    from tmlibrary_amd import hip
    lib = hip.load_library()
    for n in (0, 1, 65535, 65536, 131071, 43200, 1 << 20):
        assert lib.tmh_deflate_bound(n) == dc.bound(n)
    assert lib.tmh_deflate_scratch_bytes(0, 43200) == 0
    assert lib.tmh_deflate_scratch_bytes(256, 43200) >= 256 * dc.bound(43200)
    tot = C.c_int64()
    one = C.c_void_p(16)  # never dereferenced: the argument checks come first
    assert lib.tmh_gather_chunks_device(None, 1, 8, 8, 2, 4, 4, None, None, None) == hip.TMH_EINVAL
    assert b"NULL" in lib.tmh_last_error()
    assert lib.tmh_gather_chunks_device(one, 1, 8, 8, 4, 4, 4, one, one, None) == hip.TMH_EINVAL
    assert lib.tmh_deflate_device(None, 0, None, 1, 16, None, 0, None, 0, None, None,
                                  None) == hip.TMH_EINVAL
    assert b"NULL" in lib.tmh_last_error()
    assert lib.tmh_zproject_max_device(None, 1, 1, 8, 8, 2, None, None) == hip.TMH_EINVAL
    assert lib.tmh_zproject_max_device(one, 1, 0, 8, 8, 2, one, None) == hip.TMH_EINVAL
    assert lib.tmh_zproject_max(None, 1, 1, 8, 8, 2, None) == hip.TMH_EINVAL
    assert lib.tmh_deflate_images(None, 1, 8, 8, 2, 4, 4, None, None, 0, None,
                                  C.byref(tot)) == hip.TMH_EINVAL


def _host_table(exe, tmp_path, images, cr, cc):
    from tmlibrary_amd.models.file import CHUNK_DTYPE
    raws, rows = [], []
    for i, img in enumerate(images):
        k = 0
        for r0 in range(0, img.shape[0], cr):
            for c0 in range(0, img.shape[1], cc):
                rows.append((i, r0, c0))
                k += 1
        raws += dc.chunkify(img, cr, cc)
    out = dc.run_harness(exe, tmp_path, raws)
    table = np.zeros(len(raws), CHUNK_DTYPE)
    off = 0
    for k, (s, (i, r0, c0)) in enumerate(zip(out, rows)):
        table[k] = (off, len(s), k * len(raws[k]), len(raws[k]), i, r0, c0, 0, 0)
        off += len(s)
    return np.frombuffer(b"".join(out), np.uint8), table


@pytest.mark.parametrize("shape,dtype,chunks", [((37, 53), np.uint16, (16, 16)),
                                                ((20, 30), np.uint8, (20, 30)),
                                                ((270, 320), np.uint16, (135, 160))])
def test_raw_chunk_files(exe, tmp_path, monkeypatch, shape, dtype, chunks):
    """tmh5_write_channel_images_raw_chunks fed host-core streams: the files
    read back through H5Dread and through the GPU reader's strict parse."""
    from tmlibrary_amd.models import file as F
    rng = np.random.default_rng(7)
    images = [(rng.integers(0, 50, shape) * 37 % np.iinfo(dtype).max).astype(dtype)
              for _ in range(3)]
    blob, table = _host_table(exe, tmp_path, images, *chunks)
    paths = [str(tmp_path / ("site_%d.h5" % i)) for i in range(3)]
    perm = rng.permutation(len(table))  # the table may come in any order
    F.write_raw_chunks(paths, shape[0], shape[1], 8 * np.dtype(dtype).itemsize, chunks[0],
                       chunks[1], blob, table[perm], n_threads=2)
    for p, img in zip(paths, images):
        got = F.read_channel_image(p)
        assert got.dtype == img.dtype and np.array_equal(got, img)
    monkeypatch.setenv("TMH5_CHUNK_INDEX", "parse")  # no libhdf5 fallback
    blob2, table2, geom = F.read_raw_chunks(paths, n_threads=2)
    assert geom == (shape[0], shape[1], np.dtype(dtype).itemsize, chunks[0], chunks[1])
    assert len(table2) == len(table)
    for a, b in zip(table, table2):
        assert (a["image"], a["row0"], a["col0"], a["src_len"]) == \
               (b["image"], b["row0"], b["col0"], b["src_len"])
        assert bytes(blob[a["src_off"]:a["src_off"] + a["src_len"]]) == \
               bytes(blob2[b["src_off"]:b["src_off"] + b["src_len"]])
    with pytest.raises(ValueError):
        F.write_raw_chunks(paths, shape[0], shape[1], 8 * np.dtype(dtype).itemsize, chunks[0],
                           chunks[1], blob, table[:-1])
