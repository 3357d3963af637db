"""GPU PNG encode of channel images (ChannelImage.png_encode, png_encode_sites).

The reference codes a site with cv2.imencode('.png') (tmlib/image.py:672-682).
Bars: the kernels' files are the bytes of the host build of the same core
(tests/png_host.cpp, checked against Pillow, zlib and the numpy restatement in
test_png_cpu.py), and Pillow decodes every file to the input pixels.  The
coder runs at two workgroup widths, 256 threads in k_png_pieces (wave-wide row
filters) and one thread in png_host: the equality of their bytes is the check
that no byte depends on the width.
"""
import ctypes as C
import io

import numpy as np
import pytest
from PIL import Image

import png_cases as pc
from tmlibrary_amd import hip
from util import load_golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    return hip.lib()


@pytest.fixture(scope="module")
def host_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("png_host")
    return pc.run_harness(pc.build_harness(str(d / "png_host")), d, [a for _, a in pc.cases()])


@pytest.fixture(scope="module")
def device_files():
    from tmlibrary_amd.image import png_encode_sites
    return [png_encode_sites(a) for _, a in pc.cases()]


def decode(f):
    im = Image.open(io.BytesIO(f))
    im.load()
    return np.array(im)


def test_device_bytes_equal_host_core(L, host_files, device_files):
    bad = [name for (name, _), enc, want in zip(pc.cases(), device_files, host_files)
           if list(enc) != want]
    assert not bad, bad


def test_offsets_and_bound(L, device_files):
    for (name, a), enc in zip(pc.cases(), device_files):
        n, h, w = a.shape
        off = enc.offsets
        assert len(enc) == n and off.dtype == np.int64 and off[0] == 0, name
        assert np.all(np.diff(off) > 0) and off[n] == enc.blob.size, name
        assert np.diff(off).max() <= L.tmh_png_bound(h, w, a.itemsize), name


def test_pillow_decodes_to_the_input(device_files):
    for (name, a), enc in zip(pc.cases(), device_files):
        for i in range(0, len(enc), max(1, len(enc) // 8)):
            got = decode(enc.file(i))
            assert got.shape == a[i].shape and np.array_equal(got.astype(a.dtype), a[i]), (name, i)


def test_two_runs_give_the_same_bytes(device_files):
    from tmlibrary_amd.image import png_encode_sites
    for (name, a), enc in list(zip(pc.cases(), device_files))[-4:]:  # the edge case, both batches, plaid
        again = png_encode_sites(a)
        assert np.array_equal(again.offsets, enc.offsets) and np.array_equal(again.blob, enc.blob), name


def test_channel_image_png_encode(L):
    from tmlibrary_amd.image import ChannelImage, png_encode_sites
    for name in ("smooth_v16", "edge_1", "3x5_u8"):
        a = dict(pc.cases())[name][0]
        got = ChannelImage(a).png_encode()
        assert got.dtype == np.uint8 and got.ndim == 1
        assert got.tobytes() == png_encode_sites(a).file(0), name
    img = ChannelImage(np.zeros((4, 4), np.uint16))
    img._array = np.zeros((4, 4), np.float32)  # past the setter's check
    with pytest.raises(TypeError):
        img.png_encode()
    with pytest.raises(TypeError):
        png_encode_sites(np.zeros((2, 4, 4), np.int32))
    with pytest.raises(ValueError):
        png_encode_sites(np.zeros((2, 2, 4, 4), np.uint8))
    assert len(png_encode_sites(np.zeros((0, 4, 4), np.uint8))) == 0


def test_device_tensor_input(device_files):
    import torch

    from tmlibrary_amd.image import png_encode_sites
    cs = dict(pc.cases())
    for name, view, tdt in (("batch3", np.int16, torch.int16), ("batch520", np.uint8, torch.uint8)):
        a = cs[name]
        t = torch.from_numpy(a.view(view)).to("cuda")
        enc = png_encode_sites(t)
        want = device_files[[n for n, _ in pc.cases()].index(name)]
        assert t.dtype == tdt and np.array_equal(enc.offsets, want.offsets)
        assert np.array_equal(enc.blob, want.blob), name
    one = png_encode_sites(torch.from_numpy(cs["plaid"][0]).to("cuda"))  # [H, W]
    assert len(one) == 1 and np.array_equal(decode(one.file(0)), cs["plaid"][0])
    with pytest.raises(TypeError):
        png_encode_sites(torch.zeros((1, 4, 4), dtype=torch.float32, device="cuda"))


def test_chain_sites_to_png(L):
    """The path a site takes out of TissueMAPS: correct -> align -> clip -> scale
    (Corrector.chain_u8), then the PNG file, which decodes to the chain's bytes."""
    from tmlibrary_amd.image import Corrector, align_window, png_encode_sites
    g = load_golden("chain")
    wins = np.stack([align_window(g["images"].shape[1:], y, x, *g["residues"], crop=False)[0]
                     for y, x in g["shifts"]])
    u8 = Corrector(g["smooth_mean"], g["smooth_std"]).chain_u8(g["images"][:2], wins[:2],
                                                              int(g["clip_lo"]), int(g["clip_hi"]))
    enc = png_encode_sites(u8)
    assert len(enc) == 2
    for site, f in zip(u8, enc):
        got = decode(f)
        assert got.dtype == np.uint8 and np.array_equal(got, site)


def test_host_form_short_capacity(L):
    a = dict(pc.cases())["smooth_u8_v16"]
    n, h, w = a.shape
    offs = np.zeros(n + 1, np.int64)
    tot = C.c_int64(0)
    blob = np.zeros(int(L.tmh_png_bound(h, w, 1)), np.uint8)
    hip.check(L.tmh_png_encode(hip.ptr(a), n, h, w, 1, hip.ptr(blob), blob.nbytes, hip.ptr(offs),
                               C.byref(tot)))
    size = tot.value
    assert 0 < size == offs[1] and np.array_equal(decode(blob[:size].tobytes()), a[0])
    tot = C.c_int64(0)
    assert L.tmh_png_encode(hip.ptr(a), n, h, w, 1, hip.ptr(blob), size - 1, hip.ptr(offs),
                            C.byref(tot)) == hip.TMH_EINVAL
    assert tot.value == size and b"capacity" in L.tmh_last_error()
