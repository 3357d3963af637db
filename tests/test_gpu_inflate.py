"""GPU inflate of HDF5 gzip chunks (the site-image input path).

The reference reads sites through h5py, whose deflate filter is zlib's inflate
(tmlib/models/file.py:322-351, tmlib/readers.py:367-389).  Bar: every chunk
decoded by tmh_inflate_device is byte-identical to ``zlib.decompress`` of the
same stream -- zlib (Python's stdlib binding of the library libhdf5 links) is
the oracle -- over every deflate block kind (stored, fixed, dynamic; the
strategies and window sizes zlib can emit), and corrupt streams are reported
per chunk (TMH_Z_*) without touching other chunks.  Then whole channel image
files: DeviceChunkDecoder on files written through libtmh5 (whole-row and
2-D chunks with edge padding, uint8 and uint16, several levels) equals the
host read (libhdf5 + zlib), and at full size (2160x2560 synthetic sites).

The hand-built streams of tests/inflate_cases.py -- what the format allows and
zlib's encoder never emits, the dependency patterns of the match resolver
(k_resolve_matches has no host twin), one stream per status clause, every
bit flip and truncation of four seeds, odd layouts -- run through the device
at every workgroup width; tests/test_inflate_host.py runs the same cases
through the host build of the core under the sanitizers.  tmh_place_chunks_device
is checked alone against numpy slice assignment.
"""
import os
import zlib

import numpy as np
import pytest

import inflate_cases as ic
from tmlibrary_amd import hip
from util import keep  # noqa: F401 (a fixture)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    return hip.lib()


def _streams():
    """(name, raw bytes, zlib stream) for every block kind zlib produces."""
    rng = np.random.default_rng(5)
    from tmlibrary_amd.synth import synth_exact_host
    site = synth_exact_host(64, 512, 12345, 0, 3)  # microscopy-like u16 rows
    data = {
        "site_rows": site.tobytes(),
        "random": rng.integers(0, 256, 40000, dtype=np.uint8).tobytes(),
        "zeros": bytes(70000),
        "ramp": (np.arange(30000, dtype=np.uint16) // 7).tobytes(),
        "repeat3": b"abc" * 20000,  # overlapping back-references (distance < length)
        "one": b"\x07",
        "text": (b"corilla illumination statistics " * 900),
    }
    out = []
    for name, raw in data.items():
        for lvl in (0, 1, 4, 9):
            out.append(("%s_l%d" % (name, lvl), raw, zlib.compress(raw, lvl)))
        for strat, sname in ((zlib.Z_FILTERED, "filtered"), (zlib.Z_HUFFMAN_ONLY, "huffman"),
                             (zlib.Z_RLE, "rle"), (zlib.Z_FIXED, "fixed")):
            co = zlib.compressobj(6, zlib.DEFLATED, 15, 8, strat)
            out.append(("%s_%s" % (name, sname), raw, co.compress(raw) + co.flush()))
        for wbits in (9, 12):
            co = zlib.compressobj(6, zlib.DEFLATED, wbits, 1)
            out.append(("%s_w%d" % (name, wbits), raw, co.compress(raw) + co.flush()))
        # several blocks with sync / full flushes between them (empty stored blocks)
        co = zlib.compressobj(4)
        h = len(raw) // 3
        s = co.compress(raw[:h]) + co.flush(zlib.Z_SYNC_FLUSH)
        s += co.compress(raw[h:2 * h]) + co.flush(zlib.Z_FULL_FLUSH) + co.compress(raw[2 * h:])
        out.append(("%s_flushes" % name, raw, s + co.flush()))
    return out


def _run(L, streams, raw_lens=None):
    """tmh_inflate_device over the streams as one launch; returns (outputs, statuses)."""
    n = len(streams)
    blob = b"".join(s for _, _, s in streams)
    tab = np.zeros(n, hip.ZCHUNK_DTYPE)
    off = roff = 0
    for i, (_, raw, s) in enumerate(streams):
        rl = len(raw) if raw_lens is None else raw_lens[i]
        tab[i] = (off, len(s), roff, rl, i, 0, 0, 0, 0)
        off += len(s)
        roff += rl
    raw_max = int(tab["raw_len"].max())
    scr = int(L.tmh_inflate_scratch_bytes(n, raw_max))
    with hip.DeviceBuffer(max(len(blob), 1)) as d_src, hip.DeviceBuffer(tab.nbytes) as d_tab, \
            hip.DeviceBuffer(max(roff, 1)) as d_raw, hip.DeviceBuffer(4 * n) as d_st, \
            hip.DeviceBuffer(max(scr, 1)) as d_scr:
        d_src.put(np.frombuffer(blob, np.uint8))
        d_tab.put(tab)
        hip.check(L.tmh_inflate_device(d_src, len(blob), d_tab, n, raw_max, d_raw, roff,
                                       d_scr, scr, d_st, None))
        assert L.tmh_synchronize(None) == 0
        rawout = d_raw.get((max(roff, 1),), np.uint8)
        st = d_st.get((n,), np.int32)
    outs = [rawout[t["raw_off"]:t["raw_off"] + t["raw_len"]].tobytes() for t in tab]
    return outs, st


@pytest.mark.parametrize("lanes", [None, 4, 64])
def test_inflate_every_block_kind_bit_exact(L, monkeypatch, lanes):
    """Every workgroup width the phase-1 launch can pick decodes the same."""
    if lanes:
        monkeypatch.setenv("TMH_INFLATE_LANES", str(lanes))
    streams = _streams()
    outs, st = _run(L, streams)
    bad = [(name, int(s)) for (name, _, _), s in zip(streams, st) if s]
    assert not bad, bad
    for (name, raw, s), got in zip(streams, outs):
        assert got == zlib.decompress(s) == raw, name


def test_inflate_many_streams_one_launch(L):
    """More streams than one workgroup's lanes, each its own content."""
    rng = np.random.default_rng(8)
    streams = []
    for i in range(300):
        raw = (rng.integers(0, 600 + 40 * i, 900 + 37 * i, dtype=np.uint16)).tobytes()
        streams.append(("s%d" % i, raw, zlib.compress(raw, (i % 9) + 1)))
    outs, st = _run(L, streams)
    assert not np.any(st)
    for (name, raw, s), got in zip(streams, outs):
        assert got == raw, name


def test_inflate_corrupt_streams_reported(L):
    """Corrupt chunks get their own status; the good chunks of the same
    launch still decode exactly."""
    raw = (np.arange(20000, dtype=np.uint16) % 1234).tobytes()
    good = zlib.compress(raw, 6)
    flipped = bytearray(good)
    flipped[len(good) // 2] ^= 0x5A
    bad_adler = good[:-1] + bytes([good[-1] ^ 1])
    streams = [
        ("good", raw, good),
        ("truncated", raw, good[: len(good) // 2]),
        ("bad_adler", raw, bad_adler),
        ("flipped", raw, bytes(flipped)),
        ("not_zlib", raw, b"\x1f\x8b" + good[2:]),
        ("good2", raw, good),
    ]
    raw_lens = [len(raw)] * 6
    outs, st = _run(L, streams, raw_lens)
    assert st[0] == 0 and st[5] == 0
    assert outs[0] == raw and outs[5] == raw
    assert st[1] != 0 and st[2] == 7 and st[3] != 0 and st[4] == 1
    # wrong expected sizes: too small -> overflow, too large -> size
    outs, st = _run(L, [("small", raw, good), ("large", raw, good)], [len(raw) - 10, len(raw) + 10])
    assert st[0] == 5 and st[1] == 8
    assert set(hip.Z_STATUS) >= set(int(x) for x in st)


def _files(tmp_path, n, H, W, dtype, chunks, level, seed=1):
    from tmlibrary_amd.models.file import write_channel_image
    from tmlibrary_amd.synth import synth_exact_host
    paths, imgs = [], []
    for i in range(n):
        a = synth_exact_host(H, W, seed, 0, i)
        if dtype == np.uint8:
            a = (a >> 4).astype(np.uint8)
        p = os.path.join(str(tmp_path), "channel_image_file_%d.h5" % i)
        write_channel_image(p, a, level, chunks=chunks)
        paths.append(p)
        imgs.append(a)
    return paths, np.stack(imgs)


@pytest.mark.parametrize("H,W,dtype,chunks,level", [
    (300, 500, np.uint16, None, 4),        # h5py's default chunks (38 x 125), last row padded
    (300, 500, np.uint16, (64, 96), 1),    # 2-D chunks, right and bottom edges padded
    (257, 333, np.uint8, (50, 50), 9),
    (128, 256, np.uint16, (128, 256), 6),  # one chunk per file
])
def test_device_decode_channel_image_files(L, tmp_path, H, W, dtype, chunks, level):
    import torch

    from tmlibrary_amd.models.device_decode import DeviceChunkDecoder
    from tmlibrary_amd.models.file import read_channel_image
    paths, want = _files(tmp_path, 5, H, W, dtype, chunks, level)
    for p, w in zip(paths, want):
        assert np.array_equal(read_channel_image(p), w)  # the host path reads what was written
    tdt = torch.int16 if dtype == np.uint16 else torch.uint8
    out = torch.empty((5, H, W), dtype=tdt, device="cuda")
    dec = DeviceChunkDecoder(n_threads=4)
    assert dec.decode(paths, out.data_ptr()) == (H, W, np.dtype(dtype).itemsize)
    dec.check()
    torch.cuda.synchronize()
    got = out.cpu().numpy().view(dtype)
    assert np.array_equal(got, want)
    # the same decoder again (slot reuse), a different subset of the files
    out2 = torch.empty((3, H, W), dtype=tdt, device="cuda")
    dec.decode(paths[1:4], out2.data_ptr())
    dec.decode(paths[:3], out.data_ptr())
    dec.check()
    torch.cuda.synchronize()
    assert np.array_equal(out2.cpu().numpy().view(dtype), want[1:4])
    assert np.array_equal(out.cpu().numpy().view(dtype)[:3], want[:3])


@pytest.mark.timeout(300)
def test_device_decode_fullsize_sites(L, tmp_path):
    """Eight 2160x2560 synthetic sites, written as the reference-layout files
    (gzip level 4, h5py's default 135 x 160 chunks), decoded on the GPU = the host read."""
    import torch

    from tmlibrary_amd.models.device_decode import DeviceChunkDecoder
    paths, want = _files(tmp_path, 8, 2160, 2560, np.uint16, None, 4, seed=12345)
    out = torch.empty((8, 2160, 2560), dtype=torch.int16, device="cuda")
    dec = DeviceChunkDecoder()
    dec.decode(paths, out.data_ptr())
    dec.check()
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.uint16), want)


def test_corrupt_file_raises(L, tmp_path):
    """A damaged chunk on disk: the decoder's check names the file and the
    reason (zlib would raise on the same bytes)."""
    import torch

    from tmlibrary_amd.models.device_decode import DeviceChunkDecoder
    from tmlibrary_amd.models.file import read_raw_chunks
    paths, _ = _files(tmp_path, 2, 200, 300, np.uint16, (50, 300), 4)
    blob, table, _ = read_raw_chunks(paths[1:])
    e = table[2]
    chunk = blob[e["src_off"]:e["src_off"] + e["src_len"]].tobytes()
    data = bytearray(open(paths[1], "rb").read())
    at = data.find(chunk)
    assert at > 0 and data.find(chunk, at + 1) < 0
    data[at + len(chunk) // 2] ^= 0xFF
    data[at + len(chunk) - 1] ^= 0x01  # the Adler-32 too
    open(paths[1], "wb").write(bytes(data))
    with pytest.raises(zlib.error):
        zlib.decompress(bytes(data[at:at + len(chunk)]))
    out = torch.empty((2, 200, 300), dtype=torch.int16, device="cuda")
    dec = DeviceChunkDecoder(n_threads=2)
    dec.decode(paths, out.data_ptr())
    with pytest.raises(IOError, match="channel_image_file_1.h5: chunk 6"):
        dec.check()


# ---- the hand-built families (tests/inflate_cases.py)

class _Device:
    """Launches of tmh_inflate_device on device buffers that only grow."""

    def __init__(self, L):
        self.L, self.bufs = L, {}

    def buf(self, key, nbytes):
        b = self.bufs.get(key)
        if b is None or b.nbytes < nbytes:
            if b is not None:
                b.free()
            b = self.bufs[key] = hip.DeviceBuffer(max(nbytes, 1) * 2)
        return b

    def run(self, blob, rows, raw_bytes):
        """The whole raw buffer (pre-filled with the sentinel) and the statuses."""
        from test_inflate_host import table_of
        L, n = self.L, len(rows)
        tab = table_of(rows)
        raw_max = int(tab["raw_len"].max())
        scr = int(L.tmh_inflate_scratch_bytes(n, raw_max))
        d_src, d_tab = self.buf("src", len(blob)), self.buf("tab", tab.nbytes)
        d_raw, d_st, d_scr = self.buf("raw", raw_bytes), self.buf("st", 4 * n), self.buf("scr", scr)
        if blob:
            d_src.put(np.frombuffer(blob, np.uint8))
        d_tab.put(tab)
        d_raw.put(np.full(max(raw_bytes, 1), ic.SENTINEL, np.uint8))
        d_st.put(np.full(n, 0x7F7F7F7F, np.int32))
        hip.check(L.tmh_inflate_device(d_src, len(blob), d_tab, n, raw_max, d_raw, raw_bytes,
                                       d_scr, scr, d_st, None))
        assert L.tmh_synchronize(None) == 0
        return d_raw.get((max(raw_bytes, 1),), np.uint8)[:raw_bytes], d_st.get((n,), np.int32)

    def free(self):
        for b in self.bufs.values():
            b.free()


@pytest.fixture(scope="module")
def dev(L):
    d = _Device(L)
    yield d
    d.free()


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    from test_inflate_host import build_harness
    return build_harness(tmp_path_factory.mktemp("inflate_host"), False)


def _check_launches(dev, named):
    for name, cases, kw in named:
        blob, rows, raw_bytes = ic.layout(cases, **kw)
        raw, st = dev.run(blob, rows, raw_bytes)
        ic.check_outputs(cases, rows, raw, st, name)


@pytest.mark.parametrize("family", ["A", "B", "C"])
@pytest.mark.parametrize("lanes", [None, 4, 64])
def test_hand_built_family_on_device(dev, monkeypatch, lanes, family):
    """A: distance 32768, every length and distance symbol at both ends of its
    extra bits, codes of 1..15 bits, repeat codes across the literal/distance
    boundary, the incomplete codes zlib allows, empty and stored blocks.
    B: every length 3..258 at the distances where the resolver's copy changes
    form, 300 token streams whose matches' sources end at, one byte inside, or
    63/64 matches behind an earlier destination, and the longest match lists
    (each also launched alone: raw_max its own raw_len).  C: the exact status
    of every clause, nothing written past the fault.  Bytes no chunk owns
    keep the sentinel."""
    if lanes:
        monkeypatch.setenv("TMH_INFLATE_LANES", str(lanes))
    cases = ic.families()[family]
    named = [(family, cases, {})]
    named += [(c.name, [c], {}) for c in cases if c.name.startswith("cap_")]
    _check_launches(dev, named)


@pytest.mark.parametrize("lanes", [None, 4, 64])
def test_layouts_on_device(dev, monkeypatch, lanes):
    """One stream at source offsets 0..39 x output offsets 0/1/5/15 x 0/1/15/16/17
    bytes behind it in the buffer; launches of 1, W - 1, W, W + 1 streams;
    failing, short and long streams mixed in the workgroups; stored
    (TMH_ZCHUNK_STORED) chunks at odd offsets between deflated ones."""
    if lanes:
        monkeypatch.setenv("TMH_INFLATE_LANES", str(lanes))
    _check_launches(dev, ic.family_e())


def test_invalid_streams_device_equals_host_core(dev, host_exe, tmp_path):
    """Families C and D (every bit flip and truncation, none left out): the
    outcome zlib dictates, and beyond it the device's status and every byte
    of the raw buffer -- what a failing chunk wrote before its fault
    included -- equal the host build of the same core."""
    from test_inflate_host import run_batch
    fam = ic.families()
    groups = [fam["C"]] + ic.split_launches(fam["D"])
    lay = [ic.layout(g) for g in groups]
    host = run_batch(host_exe, tmp_path, lay)
    for i, (g, (blob, rows, raw_bytes), (h_raw, h_st)) in enumerate(zip(groups, lay, host)):
        raw, st = dev.run(blob, rows, raw_bytes)
        ic.check_outputs(g, rows, raw, st, "launch %d" % i)
        diff = [(c.name, int(a), int(b)) for c, a, b in zip(g, st, h_st) if a != b]
        assert not diff, "(name, device, host): %s" % diff[:20]
        assert np.array_equal(raw, h_raw), "launch %d: raw bytes differ from the host core's" % i


@pytest.mark.parametrize("H,W,dtype,cr,cc,shift", [
    (40, 72, np.uint16, 16, 32, 0),   # 16-byte path; right-edge chunks place 8 columns, bottom clipped
    (40, 72, np.uint16, 16, 32, 2),   # the same from raw offsets that are not 16-byte aligned
    (33, 70, np.uint16, 16, 32, 0),   # row stride 140 bytes: the byte path, both edges clipped
    (48, 80, np.uint8, 16, 16, 0),
    (17, 20, np.uint32, 8, 8, 0),
    (16, 32, np.uint16, 16, 32, 0),   # one chunk per image
])
def test_place_chunks_against_slice_assignment(L, keep, H, W, dtype, cr, cc, shift):
    """tmh_place_chunks_device on a raw buffer of known bytes equals numpy
    slice assignment; a chunk left out of the table leaves its pixels alone,
    and so does the border around the images."""
    rng = np.random.default_rng(H * W + shift)
    es, n_img, border = np.dtype(dtype).itemsize, 3, 64
    grid = [(i, r, c) for i in range(n_img) for r in range(0, H, cr) for c in range(0, W, cc)]
    order = rng.permutation(len(grid))  # raw order is not image order
    chunks = rng.integers(0, 256, (len(grid), cr * cc * es), dtype=np.uint8)
    chunks[chunks == ic.SENTINEL] = 0
    tab = np.zeros(len(grid), hip.ZCHUNK_DTYPE)
    raw = np.full(shift + chunks.size + 16, 0x11, np.uint8)
    want = np.full((n_img, H, W * es), ic.SENTINEL, np.uint8)
    skipped = len(grid) // 2 if len(grid) > n_img else -1
    for k, g in enumerate(order):
        i, r, c = grid[g]
        off = shift + k * chunks.shape[1]
        raw[off:off + chunks.shape[1]] = chunks[g]
        tab[g] = (0, 0, off, chunks.shape[1], i, r, c, 0, 0)
        if g != skipped:
            rows, cols = min(cr, H - r), min(cc, W - c)
            want[i, r:r + rows, c * es:(c + cols) * es] = chunks[g].reshape(cr, cc * es)[:rows, :cols * es]
    tab = np.delete(tab, skipped) if skipped >= 0 else tab
    d_raw, d_tab = keep(hip.DeviceBuffer(raw.nbytes)), keep(hip.DeviceBuffer(tab.nbytes))
    d_img = keep(hip.DeviceBuffer(want.size + 2 * border))
    d_raw.put(raw)
    d_tab.put(tab)
    d_img.put(np.full(want.size + 2 * border, ic.SENTINEL, np.uint8))
    hip.check(L.tmh_place_chunks_device(d_raw, d_tab, len(tab), H, W, es, cr, cc,
                                        d_img.at(border), None))
    assert L.tmh_synchronize(None) == 0
    got = d_img.get((want.size + 2 * border,), np.uint8)
    assert np.all(got[:border] == ic.SENTINEL) and np.all(got[-border:] == ic.SENTINEL)
    assert np.array_equal(got[border:-border].reshape(want.shape), want)
    if skipped >= 0:
        assert np.any(want == ic.SENTINEL)
