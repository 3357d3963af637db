"""CPU: the GPU PNG encoder's core, built for the host, against Pillow and zlib.

tmlibrary_amd/csrc/png_core.h (over deflate_core.h) is the exact code the
kernels of png_kernels.hip run; tests/png_host.cpp compiles it with g++ as a
workgroup of one thread.  Every file of the case list (tests/png_cases.py) must
be a standard PNG: Pillow -- which verifies every chunk CRC and the Adler-32
when it loads a file -- decodes it to the input pixels, and its structure is
the one DESIGN §26 lays down, checked against a numpy restatement of the rules
(tests/png_literal.py).  The reference's own bytes (cv2.imencode through
libpng, tmlib/image.py:672-682) are not the contract: a PNG that decodes to the
same pixels is.  tests/test_gpu_png.py checks that the kernels emit these bytes.
"""
import collections
import ctypes as C
import io
import os
import struct
import zlib

import numpy as np
import pytest
from PIL import Image

import png_cases as pc
import png_literal as pl
from util import REPO


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return pc.build_harness(str(tmp_path_factory.mktemp("png") / "png_host"))


@pytest.fixture(scope="module")
def files(exe, tmp_path_factory):
    """[(name, image, file)] over every image of every case"""
    cs = pc.cases()
    out = pc.run_harness(exe, tmp_path_factory.mktemp("png_run"), [a for _, a in cs])
    return [("%s[%d]" % (name, i), img, f)
            for (name, a), fs in zip(cs, out) for i, (img, f) in enumerate(zip(a, fs))]


def decode(f):
    im = Image.open(io.BytesIO(f))
    im.load()
    return im.mode, np.array(im)


def test_pillow_decodes_to_the_input(files):
    for name, img, f in files:
        mode, got = decode(f)
        assert mode == ("L" if img.dtype == np.uint8 else "I;16"), name
        assert got.shape == img.shape and np.array_equal(got.astype(img.dtype), img), name


def test_chunk_structure(files):
    P = pc.piece_bytes()
    for name, img, f in files:
        chs = pl.chunks(f)  # every CRC against zlib.crc32
        types = [t for t, _ in chs]
        assert types[0] == b"IHDR" and types[-1] == b"IEND" and chs[-1][1] == b"", name
        assert len(types) >= 4 and all(t == b"IDAT" for t in types[1:-1]), name
        assert chs[0][1] == struct.pack(">IIBBBBB", img.shape[1], img.shape[0], 8 * img.itemsize,
                                        0, 0, 0, 0), name
        want = pl.filtered_stream(img)
        assert pl.inflate_idat(chs) == want, name  # zlib checks the Adler-32
        pieces = -(-len(want) // P)
        assert len(types) - 2 == pieces + 1, name
        assert chs[1][1][:2] == b"\x78\x5e", name
        for _, body in chs[1:-3]:  # every piece but the last ends as a sync flush does
            assert body[-4:] == b"\x00\x00\xff\xff", name
        assert chs[-2][1] == struct.pack(">I", zlib.adler32(want)), name


def test_every_filter_type_is_chosen(files):
    seen = collections.Counter()
    for _, img, _ in files:
        seen.update(pl.filtered_rows(img)[0].tolist())
    assert sorted(seen) == [0, 1, 2, 3, 4], seen


def test_size_conditions(files):
    from tmlibrary_amd import hip
    lib = hip.load_library()
    by_name = {name: (img, f) for name, img, f in files}
    for name, (img, f) in by_name.items():
        assert len(f) <= lib.tmh_png_bound(img.shape[0], img.shape[1], img.itemsize), name
    # uniform random samples: every piece stored, the bound met exactly
    img, f = by_name["random[0]"]
    assert len(f) == lib.tmh_png_bound(img.shape[0], img.shape[1], img.itemsize)
    # runs of 258-byte matches at fixed distances
    for name in ("zeros[0]", "constant[0]"):
        img, f = by_name[name]
        assert len(f) < img.nbytes / 100, name
    img, f = by_name["smooth[0]"]
    b = io.BytesIO()
    Image.fromarray(img).save(b, format="PNG", compress_level=1)
    level1 = len(zlib.compress(pl.filtered_stream(img), 1))
    print("smooth: ours %d, Pillow level 1 %d (%.4f), zlib.compress(filtered, 1) %d (%.4f)"
          % (len(f), len(b.getvalue()), len(f) / len(b.getvalue()), level1, len(f) / level1))


def test_sanitizers(files, tmp_path):
    """The same stand-alone program under ASan + UBSan, once over the case list:
    a clean exit, and the bytes of the plain build."""
    san = pc.build_harness(str(tmp_path / "png_host_san"), sanitize=True)
    out = pc.run_harness(san, tmp_path, [a for _, a in pc.cases()])
    assert [f for fs in out for f in fs] == [f for _, _, f in files]


def test_bound_and_exports():
    from tmlibrary_amd import hip
    lib = hip.load_library()
    header = open(os.path.join(REPO, "include", "tmhip.h")).read()
    for name in ("tmh_png_piece_bytes", "tmh_png_bound", "tmh_png_scratch_bytes",
                 "tmh_png_encode_device", "tmh_png_encode"):
        assert name in hip.SIGNATURES and hasattr(lib, name) and name + "(" in header, name
    P = lib.tmh_png_piece_bytes()
    assert P > 0 and P % 49152 == 0
    for h, w, es in ((1, 1, 1), (97, 253, 2), (2160, 2560, 2), (96, 511, 1)):
        f = h * (1 + w * es)
        assert lib.tmh_png_bound(h, w, es) == f + 5 * (-(-f // 49152)) + 17 * (-(-f // P)) + 58
        assert lib.tmh_png_scratch_bytes(3, h, w, es) >= 3 * (f + lib.tmh_png_bound(h, w, es))
    assert lib.tmh_png_bound(0, 8, 1) == 0 and lib.tmh_png_bound(8, 8, 3) == 0
    assert lib.tmh_png_scratch_bytes(0, 8, 8, 1) == 0


def test_refusals_without_a_gpu():
    """The argument checks come before any device call; the pointers are never read."""
    from tmlibrary_amd import hip
    lib = hip.load_library()
    bound, scr = lib.tmh_png_bound(8, 8, 2), lib.tmh_png_scratch_bytes(2, 8, 8, 2)
    src, dst, off, scratch = (C.c_void_p(v) for v in (1 << 20, 2 << 20, 3 << 20, 4 << 20))

    def dev(images=src, n=2, h=8, w=8, es=2, d=dst, db=2 * bound, o=off, s=scratch, sb=scr):
        return lib.tmh_png_encode_device(images, n, h, w, es, d, db, o, s, sb, None)

    for what, kw in (
            (b"elem_bytes", dict(es=4)), (b"elem_bytes", dict(es=0)),
            (b"positive", dict(h=0)), (b"positive", dict(w=-1)), (b"negative", dict(n=-1)),
            (b"tmh_png_bound", dict(db=2 * bound - 1)),
            (b"tmh_png_scratch_bytes", dict(sb=scr - 1)),
            (b"NULL", dict(images=None)), (b"NULL", dict(d=None)), (b"NULL", dict(o=None)),
            (b"NULL", dict(s=None)),
            (b"16-byte", dict(s=C.c_void_p((4 << 20) + 8))),
            (b"overlap", dict(d=C.c_void_p((1 << 20) + 64))),
            (b"overlap", dict(s=C.c_void_p((2 << 20) + 16)))):
        assert dev(**kw) == hip.TMH_EINVAL, kw
        assert what in lib.tmh_last_error(), (kw, lib.tmh_last_error())
    tot = C.c_int64(-1)
    offs = np.zeros(2, np.int64)
    assert lib.tmh_png_encode(None, 1, 8, 8, 2, None, 0, hip.ptr(offs), C.byref(tot)) == hip.TMH_EINVAL
    assert b"NULL" in lib.tmh_last_error()
    assert lib.tmh_png_encode(hip.ptr(offs), 1, 8, 8, 3, None, 0, hip.ptr(offs),
                              C.byref(tot)) == hip.TMH_EINVAL
    assert b"elem_bytes" in lib.tmh_last_error()
    assert lib.tmh_png_encode(hip.ptr(offs), 1, 8, 8, 1, None, 0, None, None) == hip.TMH_EINVAL
