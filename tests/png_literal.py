"""A numpy restatement of the PNG encoder's rules, written from
the PNG specification and not from png_core.h: the filtered stream (five
filters, the selection rule), a walker over a file's chunks that checks every
CRC with zlib.crc32, and the inflation of the joined IDAT data (zlib checks the
Adler-32 itself)."""
import struct
import zlib

import numpy as np

SIGNATURE = b"\x89PNG\r\n\x1a\n"


def stream_rows(img):
    """[H, W * bpp] uint8: the rows' sample bytes as PNG orders them (big-endian)."""
    img = np.ascontiguousarray(img)
    assert img.ndim == 2 and img.dtype in (np.uint8, np.uint16)
    return img.astype(img.dtype.newbyteorder(">")).view(np.uint8).reshape(img.shape[0], -1)


def filtered_rows(img):
    """(types [H], filtered [H, W * bpp]): per row the filter with the smallest
    sum of v < 128 ? v : 256 - v, ties to the lowest type; the row above row 0 and
    the bytes left of a row are zeros."""
    bpp = np.dtype(img.dtype).itemsize
    raw = stream_rows(img).astype(np.int32)
    H, nb = raw.shape
    up = np.vstack([np.zeros((1, nb), np.int32), raw[:-1]])
    left = np.hstack([np.zeros((H, bpp), np.int32), raw[:, :-bpp]]) if nb > bpp else np.zeros_like(raw)
    upleft = np.hstack([np.zeros((H, bpp), np.int32), up[:, :-bpp]]) if nb > bpp else np.zeros_like(raw)
    p = left + up - upleft
    pa, pb, pc = np.abs(p - left), np.abs(p - up), np.abs(p - upleft)
    paeth = np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, up, upleft))
    cand = np.stack([raw, raw - left, raw - up, raw - ((left + up) >> 1), raw - paeth]) & 0xFF
    cost = np.where(cand < 128, cand, 256 - cand).sum(axis=2)  # [5, H]
    types = np.argmin(cost, axis=0)  # the first of equal minima
    return types.astype(np.uint8), cand[types, np.arange(H)].astype(np.uint8)


def filtered_stream(img):
    """The bytes the zlib stream of the file inflates to."""
    types, rows = filtered_rows(img)
    return np.hstack([types[:, None], rows]).tobytes()


def chunks(data):
    """[(type, data)] of a PNG file; asserts the signature, every length and CRC."""
    data = bytes(data)
    assert data[:8] == SIGNATURE
    out, at = [], 8
    while at < len(data):
        n, = struct.unpack(">I", data[at:at + 4])
        typ, body = data[at + 4:at + 8], data[at + 8:at + 8 + n]
        assert len(body) == n and at + 12 + n <= len(data)
        crc, = struct.unpack(">I", data[at + 8 + n:at + 12 + n])
        assert crc == zlib.crc32(typ + body), (typ, at)
        out.append((typ, body))
        at += 12 + n
    assert at == len(data)
    return out


def inflate_idat(chs):
    """The filtered stream of a file's chunks: every IDAT joined and inflated."""
    d = zlib.decompressobj()
    out = d.decompress(b"".join(b for t, b in chs if t == b"IDAT"))
    assert d.eof and d.unused_data == b""
    return out
