"""Baseline JPEG of one 8-bit grayscale array exactly as libjpeg writes it
(``jpeg_set_defaults``, ``JCS_GRAYSCALE``, ``jpeg_set_quality(q, TRUE)``, the
slow-integer DCT, the standard Huffman tables, no optimisation pass): a plain
numpy / Python restatement, from the array to the whole file's bytes.

It is the oracle of tests/test_jpeg_cpu.py and tests/test_gpu_jpeg.py -- a
test helper like pyramid_literal.py, not part of the package.  It is itself
pinned byte for byte to libjpeg-turbo (through Pillow) by
tests/golden/jpeg_tiles.npz.
"""
import numpy as np

# ---- tables of ITU-T T.81 Annex K -------------------------------------------------

#: K.1, luminance quantisation, natural (row-major) order
BASE_Q = np.array([
    16, 11, 10, 16, 24, 40, 51, 61,
    12, 12, 14, 19, 26, 58, 60, 55,
    14, 13, 16, 24, 40, 57, 69, 56,
    14, 17, 22, 29, 51, 87, 80, 62,
    18, 22, 37, 56, 68, 109, 103, 77,
    24, 35, 55, 64, 81, 104, 113, 92,
    49, 64, 78, 87, 103, 121, 120, 101,
    72, 92, 95, 98, 112, 100, 103, 99], dtype=np.int64)

#: natural index of the k-th coefficient in zigzag order
ZIGZAG = np.array([
    0, 1, 8, 16, 9, 2, 3, 10,
    17, 24, 32, 25, 18, 11, 4, 5,
    12, 19, 26, 33, 40, 48, 41, 34,
    27, 20, 13, 6, 7, 14, 21, 28,
    35, 42, 49, 56, 57, 50, 43, 36,
    29, 22, 15, 23, 30, 37, 44, 51,
    58, 59, 52, 45, 38, 31, 39, 46,
    53, 60, 61, 54, 47, 55, 62, 63], dtype=np.int64)

#: K.3, luminance DC: number of codes of each length 1..16, then the symbols
DC_BITS = [0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0]
DC_VALS = list(range(12))
#: K.5, luminance AC
AC_BITS = [0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D]
AC_VALS = [
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07,
    0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xA1, 0x08, 0x23, 0x42, 0xB1, 0xC1, 0x15, 0x52, 0xD1, 0xF0,
    0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0A, 0x16, 0x17, 0x18, 0x19, 0x1A, 0x25, 0x26, 0x27, 0x28,
    0x29, 0x2A, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49,
    0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69,
    0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89,
    0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7,
    0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5,
    0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA, 0xE1, 0xE2,
    0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF1, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8,
    0xF9, 0xFA]

HEADER_BYTES = 328


def _codes(bits, vals):
    """Annex C: symbol -> (code, length) of a table given as counts + symbols."""
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


DC_CODES = _codes(DC_BITS, DC_VALS)
AC_CODES = _codes(AC_BITS, AC_VALS)


def quant_table(quality):
    """jpeg_set_quality(quality, TRUE): the 64 quantisers, natural order."""
    q = min(max(int(quality), 1), 100)
    s = 5000 // q if q < 50 else 200 - 2 * q
    return np.clip((BASE_Q * s + 50) // 100, 1, 255)


def header(height, width, quality):
    """SOI .. SOS: 328 bytes, of which only H, W and the quantisers vary."""
    u16 = lambda v: bytes([v >> 8, v & 255])  # noqa: E731
    q = quant_table(quality)
    out = b"\xFF\xD8"
    out += b"\xFF\xE0" + u16(16) + b"JFIF\0" + bytes([1, 1, 0]) + u16(1) + u16(1) + bytes([0, 0])
    out += b"\xFF\xDB" + u16(67) + bytes([0]) + bytes(int(q[i]) for i in ZIGZAG)
    out += b"\xFF\xC0" + u16(11) + bytes([8]) + u16(height) + u16(width) + bytes([1, 1, 0x11, 0])
    out += b"\xFF\xC4" + u16(19 + len(DC_VALS)) + bytes([0x00]) + bytes(DC_BITS) + bytes(DC_VALS)
    out += b"\xFF\xC4" + u16(19 + len(AC_VALS)) + bytes([0x10]) + bytes(AC_BITS) + bytes(AC_VALS)
    out += b"\xFF\xDA" + u16(8) + bytes([1, 1, 0x00, 0, 63, 0])
    assert len(out) == HEADER_BYTES
    return out


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _fdct_pass(d, first):
    """One pass of jfdctint.c over the last axis of d[..., 8] (int64)."""
    F = dict(f0_298=2446, f0_390=3196, f0_541=4433, f0_765=6270, f0_899=7373, f1_175=9633,
             f1_501=12299, f1_847=15137, f1_961=16069, f2_053=16819, f2_562=20995, f3_072=25172)
    CONST_BITS, PASS1_BITS = 13, 2
    t0, t7 = d[..., 0] + d[..., 7], d[..., 0] - d[..., 7]
    t1, t6 = d[..., 1] + d[..., 6], d[..., 1] - d[..., 6]
    t2, t5 = d[..., 2] + d[..., 5], d[..., 2] - d[..., 5]
    t3, t4 = d[..., 3] + d[..., 4], d[..., 3] - d[..., 4]
    t10, t13 = t0 + t3, t0 - t3
    t11, t12 = t1 + t2, t1 - t2
    out = np.empty_like(d)
    n = CONST_BITS - PASS1_BITS if first else CONST_BITS + PASS1_BITS
    if first:
        out[..., 0] = (t10 + t11) << PASS1_BITS
        out[..., 4] = (t10 - t11) << PASS1_BITS
    else:
        out[..., 0] = _descale(t10 + t11, PASS1_BITS)
        out[..., 4] = _descale(t10 - t11, PASS1_BITS)
    z1 = (t12 + t13) * F["f0_541"]
    out[..., 2] = _descale(z1 + t13 * F["f0_765"], n)
    out[..., 6] = _descale(z1 - t12 * F["f1_847"], n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * F["f1_175"]
    t4, t5, t6, t7 = t4 * F["f0_298"], t5 * F["f2_053"], t6 * F["f3_072"], t7 * F["f1_501"]
    z1, z2 = -z1 * F["f0_899"], -z2 * F["f2_562"]
    z3, z4 = -z3 * F["f1_961"] + z5, -z4 * F["f0_390"] + z5
    out[..., 7] = _descale(t4 + z1 + z3, n)
    out[..., 5] = _descale(t5 + z2 + z4, n)
    out[..., 3] = _descale(t6 + z2 + z3, n)
    out[..., 1] = _descale(t7 + z1 + z4, n)
    return out


def coefficients(array, quality):
    """[block rows][block cols][64] quantised coefficients, natural order."""
    a = np.asarray(array)
    assert a.dtype == np.uint8 and a.ndim == 2 and a.size > 0
    h, w = a.shape
    a = np.pad(a, ((0, -h % 8), (0, -w % 8)), mode="edge").astype(np.int64) - 128
    bh, bw = a.shape[0] // 8, a.shape[1] // 8
    d = a.reshape(bh, 8, bw, 8).transpose(0, 2, 1, 3)           # [bh][bw][row][col]
    d = _fdct_pass(d, True)                                       # rows
    d = _fdct_pass(d.transpose(0, 1, 3, 2), False).transpose(0, 1, 3, 2)   # columns
    x = d.reshape(bh, bw, 64)
    qv = 8 * quant_table(quality)
    return np.sign(x) * ((np.abs(x) + (qv >> 1)) // qv)


class _Bits(object):
    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def put(self, code, length):
        self.acc = (self.acc << length) | code
        self.n += length
        while self.n >= 8:
            b = (self.acc >> (self.n - 8)) & 255
            self.out.append(b)
            if b == 255:
                self.out.append(0)
            self.n -= 8
        self.acc &= (1 << self.n) - 1

    def flush(self):
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)


def _value_bits(v):
    """(category, the category's low bits) of a DC difference / AC coefficient."""
    size = int(abs(v)).bit_length()
    return size, (v if v >= 0 else v - 1) & ((1 << size) - 1)


def encode(array, quality=95):
    """The whole JPEG file of a uint8 [h][w] array, 1 <= h, w <= 65535."""
    a = np.asarray(array)
    coef = coefficients(a, quality)
    bits, pred = _Bits(), 0
    for block in coef.reshape(-1, 64)[:, ZIGZAG].tolist():
        size, low = _value_bits(block[0] - pred)
        pred = block[0]
        bits.put(*DC_CODES[size])
        bits.put(low, size)
        run = 0
        for v in block[1:]:
            if v == 0:
                run += 1
                continue
            while run > 15:
                bits.put(*AC_CODES[0xF0])
                run -= 16
            size, low = _value_bits(v)
            bits.put(*AC_CODES[run << 4 | size])
            bits.put(low, size)
            run = 0
        if run:
            bits.put(*AC_CODES[0x00])
    bits.flush()
    return header(a.shape[0], a.shape[1], quality) + bytes(bits.out) + b"\xFF\xD9"


# ---- the case kinds the tests share ------------------------------------------------

def case_array(kind, shape=(256, 256), seed=0):
    """A uint8 array of one of the named kinds (deterministic)."""
    h, w = shape
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    if kind == "zeros":
        a = np.zeros(shape)
    elif kind == "full":
        a = np.full(shape, 255)
    elif kind == "noise":
        a = rng.integers(0, 256, shape)
    elif kind == "cells":
        a = np.zeros(shape)
        for _ in range(max(1, h * w // 2000)):
            cy, cx, r = rng.uniform(0, h), rng.uniform(0, w), rng.uniform(3, 12)
            a += rng.lognormal(4.0, 0.6) * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * r * r))
        a = np.clip(a + rng.normal(8, 2, shape), 0, 255)
    elif kind == "checker1":
        a = ((yy + xx) & 1) * 255
    elif kind == "checker8":
        a = (((yy >> 3) + (xx >> 3)) & 1) * 255
    elif kind == "stripes":
        a = (xx & 1) * 255
    elif kind == "impulses":
        a = ((yy % 8 == 0) & (xx % 8 == 0)) * 255
    elif kind == "specks":
        a = np.zeros(shape)
        n = max(1, h * w // 700)
        a[rng.integers(0, h, n), rng.integers(0, w, n)] = rng.integers(1, 256, n)
    elif kind == "smooth":
        a = 127.5 + 127.5 * np.sin(yy / 17.0) * np.cos(xx / 23.0)
    elif kind == "ramp":
        a = (yy + xx) * 255.0 / max(1, h + w - 2)
    else:
        raise KeyError(kind)
    return np.ascontiguousarray(np.asarray(a).astype(np.uint8))


#: (name, kind, shape, quality) of tests/golden/jpeg_tiles.npz
GOLDEN_CASES = [
    ("zeros", "zeros", (256, 256), 95),
    ("full", "full", (256, 256), 95),
    ("noise", "noise", (256, 256), 95),
    ("cells", "cells", (256, 256), 95),
    ("checker1_q100", "checker1", (256, 256), 100),
    ("checker8_q100", "checker8", (256, 256), 100),
    ("stripes", "stripes", (256, 256), 95),
    ("impulses_q100", "impulses", (256, 256), 100),
    ("specks", "specks", (256, 256), 95),
    ("noise_q1", "noise", (256, 256), 1),
    ("noise_q50", "noise", (256, 256), 50),
    ("noise_q75", "noise", (256, 256), 75),
    ("ragged_1x1", "noise", (1, 1), 95),
    ("ragged_1x256", "noise", (1, 256), 95),
    ("ragged_256x1", "noise", (256, 1), 95),
    ("ragged_7x7", "noise", (7, 7), 95),
    ("ragged_9x17", "cells", (9, 17), 95),
    ("ragged_255x256", "cells", (255, 256), 95),
    ("ragged_256x255", "noise", (256, 255), 95),
]


def load_goldens(path):
    """[(name, array, quality, Pillow's bytes)] of the golden file."""
    z = np.load(path)
    return [(name, z["in_" + name], int(z["q_" + name]), z["out_" + name].tobytes())
            for name, _, _, _ in GOLDEN_CASES]
