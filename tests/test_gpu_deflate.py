"""GPU deflate of HDF5 gzip chunks: the site-image output path (imextract).

The reference writes sites through h5py, whose deflate filter is zlib's
deflate (tmlib/models/file.py:353-363, tmlib/writers.py:384-387;
tmlib/workflow/imextract/api.py:88-157 projects and stores the planes).  Bars:
the kernel's streams are the bytes of the host build of the same core
(tests/deflate_host.cpp, checked against zlib in test_deflate_cpu.py); gather
-> deflate -> inflate -> place returns the images bit for bit; files written
through the GPU encoder read back through libhdf5 and through the GPU reader;
the z projection equals numpy; the imextract job runs end to end.
"""
import contextlib
import ctypes as C
import types
import zlib

import numpy as np
import pytest

import deflate_cases as dc
from tmlibrary_amd import hip
from util import keep  # noqa: F401 (a fixture)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    return hip.lib()


def _deflate(L, raws):
    """tmh_deflate_device over the byte strings as one launch: (streams, statuses)."""
    n = len(raws)
    tab = np.zeros(n, hip.ZCHUNK_DTYPE)
    roff = 0
    for i, r in enumerate(raws):
        tab[i] = (0, 0, roff, len(r), i, 0, 0, 0, 0)
        roff += len(r)
    raw_max = int(tab["raw_len"].max())
    dst_bytes = n * int(L.tmh_deflate_bound(raw_max))
    scr = int(L.tmh_deflate_scratch_bytes(n, raw_max))
    with contextlib.ExitStack() as stack:
        keep = stack.enter_context
        sizes = (max(roff, 1), tab.nbytes, dst_bytes, max(scr, 1), 4 * n, 8)
        d_raw, d_tab, d_dst, d_scr, d_st, d_tot = [keep(hip.DeviceBuffer(b)) for b in sizes]
        d_raw.put(np.frombuffer(b"".join(raws), np.uint8))
        d_tab.put(tab)
        hip.check(L.tmh_deflate_device(d_raw, roff, d_tab, n, raw_max, d_dst, dst_bytes,
                                       d_scr, scr, d_st, d_tot, None))
        assert L.tmh_synchronize(None) == 0
        total = int(d_tot.get((1,), np.int64)[0])
        tab = d_tab.get((n,), hip.ZCHUNK_DTYPE)
        st = d_st.get((n,), np.int32)
        blob = d_dst.get((max(total, 1),), np.uint8)
        assert total == int(tab["src_len"].sum())
        assert np.array_equal(tab["src_off"], np.concatenate([[0], np.cumsum(tab["src_len"])[:-1]]))
    return [blob[t["src_off"]:t["src_off"] + t["src_len"]].tobytes() for t in tab], st


def test_device_bytes_equal_host_core(L, tmp_path):
    cs = dc.cases()
    raws = [r for _, r in cs]
    want = dc.run_harness(dc.build_harness(str(tmp_path / "deflate_host")), tmp_path, raws)
    got, st = _deflate(L, raws)
    assert not np.any(st)
    bad = [name for (name, _), g, w in zip(cs, got, want) if g != w]
    assert not bad, bad
    for (name, raw), s in zip(cs, got):
        assert zlib.decompress(s) == raw, name
        assert len(s) <= dc.bound(len(raw)), name


def test_bad_table_entry_is_reported(L, keep):
    raw = bytes(range(200))
    tab = np.zeros(2, hip.ZCHUNK_DTYPE)
    tab[0] = (0, 0, 0, 200, 0, 0, 0, 0, 0)
    tab[1] = (0, 0, 100, 200, 1, 0, 0, 0, 0)  # runs past the raw buffer
    dst_bytes = 2 * int(L.tmh_deflate_bound(200))
    scr = int(L.tmh_deflate_scratch_bytes(2, 200))
    sizes = (200, tab.nbytes, dst_bytes, max(scr, 1), 8, 8)
    d_raw, d_tab, d_dst, d_scr, d_st, d_tot = [keep(hip.DeviceBuffer(b)) for b in sizes]
    d_raw.put(np.frombuffer(raw, np.uint8))
    d_tab.put(tab)
    hip.check(L.tmh_deflate_device(d_raw, 200, d_tab, 2, 200, d_dst, dst_bytes, d_scr, scr,
                                   d_st, d_tot, None))
    assert L.tmh_synchronize(None) == 0
    st = d_st.get((2,), np.int32)
    tab = d_tab.get((2,), hip.ZCHUNK_DTYPE)
    total = int(d_tot.get((1,), np.int64)[0])
    assert st[0] == 0 and st[1] == 6 and tab["src_len"][1] == 0 and total == tab["src_len"][0]
    assert zlib.decompress(d_dst.get((total,), np.uint8).tobytes()) == raw
    assert L.tmh_deflate_device(d_raw, 200, d_tab, 2, 200, d_dst, dst_bytes - 1, d_scr, scr,
                                d_st, d_tot, None) == hip.TMH_EINVAL


@pytest.mark.parametrize("n,H,W,dtype,chunks", [
    (2, 2160, 2560, np.uint16, (135, 160)),
    (3, 37, 53, np.uint16, (16, 16)),  # edge chunks on both axes
    (2, 20, 30, np.uint8, (20, 30)),
    (1, 1, 1, np.uint16, (1, 1)),
])
def test_device_round_trip(L, keep, n, H, W, dtype, chunks):
    """gather -> deflate -> inflate -> place returns the images bit for bit."""
    from tmlibrary_amd.synth import synth_exact_sites_host
    es = np.dtype(dtype).itemsize
    if H * W == 1:
        imgs = np.full((n, 1, 1), 0xBEEF, np.uint16)
    else:
        imgs = synth_exact_sites_host(n, H, W)
    imgs = imgs if dtype == np.uint16 else (imgs >> 3).astype(np.uint8)
    cr, cc = chunks
    nch = n * (-(-H // cr)) * (-(-W // cc))
    raw_max = cr * cc * es
    raw_bytes = nch * raw_max
    dst_bytes = nch * int(L.tmh_deflate_bound(raw_max))
    scr = max(int(L.tmh_deflate_scratch_bytes(nch, raw_max)),
              int(L.tmh_inflate_scratch_bytes(nch, raw_max)))
    sizes = (imgs.nbytes, imgs.nbytes, nch * hip.ZCHUNK_DTYPE.itemsize, raw_bytes, raw_bytes,
             dst_bytes + 16, max(scr, 1), 4 * nch, 8)
    d_img, d_out, d_tab, d_raw, d_raw2, d_dst, d_scr, d_st, d_tot = \
        [keep(hip.DeviceBuffer(b)) for b in sizes]
    d_img.put(imgs)
    d_out.put(np.full(imgs.shape, 0xA5, dtype))
    hip.check(L.tmh_gather_chunks_device(d_img, n, H, W, es, cr, cc, d_tab, d_raw, None))
    hip.check(L.tmh_deflate_device(d_raw, raw_bytes, d_tab, nch, raw_max, d_dst, dst_bytes,
                                   d_scr, scr, d_st, d_tot, None))
    assert L.tmh_synchronize(None) == 0
    assert not np.any(d_st.get((nch,), np.int32))
    total = int(d_tot.get((1,), np.int64)[0])
    tab = d_tab.get((nch,), hip.ZCHUNK_DTYPE)
    assert np.array_equal(tab["image"], np.repeat(np.arange(n), nch // n))
    assert np.all(tab["raw_len"] == raw_max) and tab["row0"].max() < H and tab["col0"].max() < W
    # the gathered chunks are HDF5's: zero padded past the extent
    raw = d_raw.get((raw_bytes,), np.uint8).tobytes()
    want = b"".join(c for img in imgs for c in dc.chunkify(img, cr, cc))
    assert raw == want
    blob = d_dst.get((max(total, 1),), np.uint8)
    for t in tab[:: max(1, nch // 16)]:  # zlib takes them too
        assert zlib.decompress(blob[t["src_off"]:t["src_off"] + t["src_len"]].tobytes()) == \
            raw[t["raw_off"]:t["raw_off"] + t["raw_len"]]
    hip.check(L.tmh_inflate_device(d_dst, total, d_tab, nch, raw_max, d_raw2, raw_bytes,
                                   d_scr, scr, d_st, None))
    hip.check(L.tmh_place_chunks_device(d_raw2, d_tab, nch, H, W, es, cr, cc, d_out, None))
    assert L.tmh_synchronize(None) == 0
    assert not np.any(d_st.get((nch,), np.int32))
    assert np.array_equal(d_out.get(imgs.shape, dtype), imgs)


@pytest.mark.parametrize("H,W,dtype,chunks", [(300, 500, np.uint16, None),
                                              (257, 333, np.uint8, (50, 50)),
                                              (37, 53, np.uint16, (64, 64))])
def test_files_written_by_the_device_encoder(L, tmp_path, monkeypatch, H, W, dtype, chunks):
    import torch

    from tmlibrary_amd.models.device_decode import DeviceChunkDecoder
    from tmlibrary_amd.models.device_encode import deflate_sites, write_channel_images_device
    from tmlibrary_amd.models.file import read_channel_image, write_channel_images
    from tmlibrary_amd.synth import synth_exact_sites_host
    want = synth_exact_sites_host(5, H, W)
    want = want if dtype == np.uint16 else (want >> 4).astype(np.uint8)
    paths = [str(tmp_path / ("site_%d.h5" % i)) for i in range(5)]
    write_channel_images_device(paths, want, chunks)  # a numpy array
    for p, w in zip(paths, want):
        got = read_channel_image(p)
        assert got.dtype == w.dtype and np.array_equal(got, w)
    monkeypatch.setenv("TMH5_CHUNK_INDEX", "parse")  # the reader's strict parse, no fallback
    tdt = torch.int16 if dtype == np.uint16 else torch.uint8
    out = torch.empty((5, H, W), dtype=tdt, device="cuda")
    dec = DeviceChunkDecoder(n_threads=4)
    assert dec.decode(paths, out.data_ptr()) == (H, W, np.dtype(dtype).itemsize)
    dec.check()
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().view(dtype), want)
    # a device tensor through the public writer, the shared encoder's slots reused
    paths2 = [str(tmp_path / ("again_%d.h5" % i)) for i in range(3)]
    write_channel_images(paths2, out[1:4], encode="gpu", chunks=chunks)
    for p, w in zip(paths2, want[1:4]):
        assert np.array_equal(read_channel_image(p), w)
    blob, table, geom = deflate_sites(want[:1], chunks)
    assert geom[:3] == (H, W, np.dtype(dtype).itemsize)
    assert len(blob) == int(table["src_len"].sum())


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
@pytest.mark.parametrize("z", [1, 2, 5])
def test_zproject_max_small(L, dtype, z):
    rng = np.random.default_rng(z)
    planes = rng.integers(0, np.iinfo(dtype).max, (3, z, 37, 53)).astype(dtype)
    out = np.empty((3, 37, 53), dtype)
    hip.check(L.tmh_zproject_max(planes.ctypes.data, 3, z, 37, 53, planes.itemsize,
                                 out.ctypes.data))
    assert np.array_equal(out, planes.max(axis=1))


def test_zproject_max_fullsize(L):
    rng = np.random.default_rng(11)
    planes = rng.integers(0, 65536, (1, 3, 2160, 2560), dtype=np.uint16)
    out = np.empty((1, 2160, 2560), np.uint16)
    hip.check(L.tmh_zproject_max(planes.ctypes.data, 1, 3, 2160, 2560, 2, out.ctypes.data))
    assert np.array_equal(out, planes.max(axis=1))
    p8 = (planes[0, :2] >> 8).astype(np.uint8)[None]
    o8 = np.empty((1, 2160, 2560), np.uint8)
    hip.check(L.tmh_zproject_max(p8.ctypes.data, 1, 2, 2160, 2560, 1, o8.ctypes.data))
    assert np.array_equal(o8, p8.max(axis=1))


def test_host_wrapper_deflate_images(L):
    from tmlibrary_amd.synth import synth_exact_sites_host
    imgs = synth_exact_sites_host(2, 37, 53)
    n = 2 * 3 * 4
    tab = np.zeros(n, hip.ZCHUNK_DTYPE)
    st = np.ones(n, np.int32)
    blob = np.zeros(n * int(L.tmh_deflate_bound(16 * 16 * 2)), np.uint8)
    tot = C.c_int64()
    hip.check(L.tmh_deflate_images(imgs.ctypes.data, 2, 37, 53, 2, 16, 16, tab.ctypes.data,
                                   blob.ctypes.data, blob.nbytes, st.ctypes.data, C.byref(tot)))
    assert not np.any(st) and tot.value == int(tab["src_len"].sum())
    want = [c for img in imgs for c in dc.chunkify(img, 16, 16)]
    for t, w in zip(tab, want):
        assert zlib.decompress(blob[t["src_off"]:t["src_off"] + t["src_len"]].tobytes()) == w


def test_imextract_job_end_to_end(L, tmp_path):
    from tmlibrary_amd.models.file import ExperimentStore, read_channel_image
    from tmlibrary_amd.synth import synth_exact_host
    from tmlibrary_amd.workflow.imextract.api import ImageExtractor
    z = 3
    maps = {fid: {"files": ["stack_%d.tif" % fid] * z, "series": [0] * z, "planes": list(range(z))}
            for fid in range(1, 9)}

    def source(filename, series, plane):
        fid = int(filename.split("_")[1].split(".")[0])
        return synth_exact_host(192, 256, site=fid * 8 + plane)
    store = ExperimentStore(str(tmp_path))
    ex = ImageExtractor(1, store, maps, source, encode="gpu")
    for batch in ex.create_run_batches(types.SimpleNamespace(batch_size=8)):
        ex.run_job(batch)
    assert ex.last_path == "gpu"
    for fid in maps:
        want = np.max(np.dstack([source("stack_%d.tif" % fid, 0, p) for p in range(z)]), 2)
        assert np.array_equal(read_channel_image(store.channel_image_file(fid).location), want)
