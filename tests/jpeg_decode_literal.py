"""What libjpeg decodes from a baseline JPEG file of one 8-bit grayscale
component (``jpeg_idct_islow``, the range limit, the crop to SOF0's size): a
plain numpy / Python restatement of DESIGN.md section 14, from the file's bytes
to the picture, and the round trip ``decode(encode(array))`` without the
entropy coding in between.

It is the oracle of tests/test_jpeg_decode_cpu.py and
tests/test_gpu_jpeg_decode.py -- a test helper like jpeg_literal.py, not part
of the package.  It is itself pinned pixel for pixel to libjpeg-turbo (through
Pillow) by tests/golden/jpeg_decoded.npz.
"""
import numpy as np

import jpeg_literal as jl

OK, UNSUPPORTED, CORRUPT = 0, 1, 2


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _idct_pass(c, n):
    """One pass of jidctint.c over the last axis of c[..., 8] (int64)."""
    z1 = (c[..., 2] + c[..., 6]) * 4433
    e2, e3 = z1 - c[..., 6] * 15137, z1 + c[..., 2] * 6270
    e0, e1 = (c[..., 0] + c[..., 4]) << 13, (c[..., 0] - c[..., 4]) << 13
    t10, t13, t11, t12 = e0 + e3, e0 - e3, e1 + e2, e1 - e2
    o0, o1, o2, o3 = c[..., 7], c[..., 5], c[..., 3], c[..., 1]
    z1, z2, z3, z4 = o0 + o3, o1 + o2, o0 + o2, o1 + o3
    z5 = (z3 + z4) * 9633
    o0, o1, o2, o3 = o0 * 2446, o1 * 16819, o2 * 25172, o3 * 12299
    z1, z2 = -z1 * 7373, -z2 * 20995
    z3, z4 = -z3 * 16069 + z5, -z4 * 3196 + z5
    o0, o1, o2, o3 = o0 + z1 + z3, o1 + z2 + z4, o2 + z2 + z3, o3 + z1 + z4
    out = np.empty_like(c)
    out[..., 0], out[..., 7] = _descale(t10 + o3, n), _descale(t10 - o3, n)
    out[..., 1], out[..., 6] = _descale(t11 + o2, n), _descale(t11 - o2, n)
    out[..., 2], out[..., 5] = _descale(t12 + o1, n), _descale(t12 - o1, n)
    out[..., 3], out[..., 4] = _descale(t13 + o0, n), _descale(t13 - o0, n)
    return out


def idct(coef):
    """[..., 64] dequantised coefficients (natural order) -> [..., 8, 8] uint8."""
    c = np.asarray(coef, dtype=np.int64).reshape(coef.shape[:-1] + (8, 8))
    c = _idct_pass(c.swapaxes(-1, -2), 13 - 2).swapaxes(-1, -2)   # pass 1: columns
    c = _idct_pass(c, 13 + 2 + 3)                                   # pass 2: rows
    return np.clip(c + 128, 0, 255).astype(np.uint8)


def _assemble(blocks, h, w):
    bh, bw = blocks.shape[:2]
    return np.ascontiguousarray(blocks.transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8)[:h, :w])


def roundtrip(array, quality=95):
    """The picture libjpeg decodes from ``jpeg_literal.encode(array, quality)``."""
    a = np.asarray(array)
    coef = jl.coefficients(a, quality) * jl.quant_table(quality)
    return _assemble(idct(coef), a.shape[0], a.shape[1])


# ---- the file ----------------------------------------------------------------------------

def _lookup(bits, vals):
    """(code, length) -> symbol."""
    return {v: k for k, v in jl._codes(bits, vals).items()}


_DC = _lookup(jl.DC_BITS, jl.DC_VALS)
_AC = _lookup(jl.AC_BITS, jl.AC_VALS)


def parse_header(f):
    """(status, height, width, quantisers in natural order, offset of the scan)."""
    n = len(f)
    bad = (CORRUPT, 0, 0, None, 0)
    if n < 4 or f[0] != 0xFF or f[1] != 0xD8:
        return bad
    unsupported = have_sof = have_dc = have_ac = False
    q, height, width, component = None, 0, 0, 0
    at = 2
    while True:
        if at + 4 > n or f[at] != 0xFF:
            return bad
        m = f[at + 1]
        length = f[at + 2] << 8 | f[at + 3]
        seg, end = at + 4, at + 2 + length
        if m in (0xFF, 0x00, 0x01) or 0xD0 <= m <= 0xD9:
            return bad
        if length < 2 or end > n:
            return bad
        if m == 0xDB:
            p = seg
            while p < end:
                pq, tq = f[p] >> 4, f[p] & 15
                if pq > 1 or tq > 3:
                    return bad
                size = 128 if pq else 64
                if p + 1 + size > end:
                    return bad
                if tq == 0:
                    if pq:
                        unsupported = True
                    else:
                        vals = np.frombuffer(bytes(f[p + 1:p + 65]), np.uint8)
                        if np.any(vals == 0):
                            return bad
                        q = np.zeros(64, dtype=np.int64)
                        q[jl.ZIGZAG] = vals
                p += 1 + size
        elif m == 0xC0:
            if have_sof or length < 8:
                return bad
            nf = f[seg + 5]
            if length != 8 + 3 * nf or nf == 0:
                return bad
            have_sof = True
            height, width = f[seg + 1] << 8 | f[seg + 2], f[seg + 3] << 8 | f[seg + 4]
            component = f[seg + 6]
            if (f[seg] != 8 or nf != 1 or f[seg + 7] != 0x11 or f[seg + 8] != 0 or
                    not 1 <= height <= 256 or not 1 <= width <= 256):
                unsupported = True
        elif (0xC1 <= m <= 0xCF and m != 0xC4) or m == 0xDC:
            if m not in (0xCC, 0xDC):
                have_sof = True
            unsupported = True
        elif m == 0xC4:
            p = seg
            while p < end:
                tc, th = f[p] >> 4, f[p] & 15
                if tc > 1 or th > 3 or p + 17 > end:
                    return bad
                bits = list(f[p + 1:p + 17])
                if sum(bits) > 256 or p + 17 + sum(bits) > end:
                    return bad
                if th == 0:
                    vals = list(f[p + 17:p + 17 + sum(bits)])
                    want = (jl.AC_BITS, jl.AC_VALS) if tc else (jl.DC_BITS, jl.DC_VALS)
                    if (bits, vals) != want:
                        unsupported = True
                    if tc:
                        have_ac = True
                    else:
                        have_dc = True
                p += 17 + sum(bits)
        elif m == 0xDD:
            if length != 4:
                return bad
            if f[seg] | f[seg + 1]:
                unsupported = True
        elif m == 0xDA:
            if not have_sof or length < 6:
                return bad
            if unsupported:
                return (UNSUPPORTED, 0, 0, None, 0)
            ns = f[seg]
            if length != 6 + 2 * ns:
                return bad
            if ns != 1:
                return (UNSUPPORTED, 0, 0, None, 0)
            if f[seg + 1] != component:
                return bad
            if (f[seg + 2], f[seg + 3], f[seg + 4], f[seg + 5]) != (0, 0, 63, 0):
                return (UNSUPPORTED, 0, 0, None, 0)
            if q is None or not have_dc or not have_ac:
                return (UNSUPPORTED, 0, 0, None, 0)
            return (OK, height, width, q, end)
        at = end


class _Corrupt(Exception):
    pass


class _Reader(object):
    """The scan's bits: 0xFF 0x00 unstuffed, ending at a marker or the file's end."""

    def __init__(self, f, at):
        bits = []
        n = len(f)
        while at < n:
            b = f[at]
            if b == 0xFF:
                if at + 1 >= n or f[at + 1] != 0:
                    break
                at += 2
            else:
                at += 1
            bits.append(b)
        self.marker_at = at
        self.bits = "".join("{:08b}".format(b) for b in bits)
        self.at = 0

    def take(self, k):
        if self.at + k > len(self.bits):
            raise _Corrupt()
        v = self.bits[self.at:self.at + k]
        self.at += k
        return int(v, 2) if k else 0

    def symbol(self, table):
        code = 0
        for length in range(1, 17):
            code = code << 1 | self.take(1)
            if (code, length) in table:
                return table[(code, length)]
        raise _Corrupt()

    def value(self, size):
        x = self.take(size)
        return x - (1 << size) + 1 if size and x < 1 << (size - 1) else x


def decode(data):
    """``(array, status)`` of a file's bytes; array is None unless status is 0."""
    f = bytes(data)
    status, h, w, q, scan = parse_header(f)
    if status:
        return None, status
    bh, bw = (h + 7) // 8, (w + 7) // 8
    coef = np.zeros((bh * bw, 64), dtype=np.int64)
    r, dc = _Reader(f, scan), 0
    try:
        for b in range(bh * bw):
            s = r.symbol(_DC)
            if s > 11:
                raise _Corrupt()
            dc += r.value(s)
            if not -2048 <= dc <= 2047:
                raise _Corrupt()
            coef[b, 0] = dc
            k = 1
            while k < 64:
                sym = r.symbol(_AC)
                run, s = sym >> 4, sym & 15
                if s == 0:
                    if run != 15:
                        break
                    k += 16
                    if k > 64:
                        raise _Corrupt()
                    continue
                k += run
                if s > 10 or k > 63:
                    raise _Corrupt()
                coef[b, jl.ZIGZAG[k]] = r.value(s)
                k += 1
        m = r.marker_at
        if len(r.bits) - r.at >= 8 or f[m:m + 2] != b"\xFF\xD9":
            raise _Corrupt()
    except _Corrupt:
        return None, CORRUPT
    return _assemble(idct((coef * q).reshape(bh, bw, 64)), h, w), OK


# ---- the stored pyramid ------------------------------------------------------------------

def stored_pyramid_literal(geometry, sites, quality):
    """Level z -> (tiles dict, rows, cols): every level below the base is the
    halving of the JPEG round trip of the level above, as the reference's
    ``ChannelLayerTile.pixels`` getter hands it to
    ``_create_lower_zoom_level_tiles``; the levels themselves are uncoded."""
    import pyramid_literal as lit
    levels = {}
    z = geometry.depth - 1
    rows, cols = geometry.dimensions[z]
    tiles = lit.level_to_dict(lit.literal_base_level(geometry, sites)[0])
    levels[z] = (tiles, rows, cols)
    while z > 0:
        if quality is not None:
            tiles = {k: roundtrip(v, quality) for k, v in tiles.items()}
        tiles, rows, cols = lit.literal_lower_level(tiles, rows, cols)
        z -= 1
        levels[z] = (tiles, rows, cols)
    return levels


# ---- goldens -----------------------------------------------------------------------------

#: (kind, quality) of the ten extra ragged tiles of tests/golden/jpeg_decoded.npz;
#: shapes are drawn from default_rng(14) in make_jpeg_decode_goldens.py
EXTRA_CASES = [("noise", 1), ("cells", 30), ("specks", 50), ("smooth", 75), ("stripes", 90),
               ("ramp", 95), ("noise", 100), ("cells", 95), ("checker1", 75), ("impulses", 30)]


def load_goldens(path):
    """[(name, input or None, quality or None, file bytes, decoded)]: Pillow's
    decode of every out_* file of jpeg_tiles.npz (their files live there), then
    the ten extra tiles."""
    import os
    z = np.load(path)
    tiles = jl.load_goldens(os.path.join(os.path.dirname(path), "jpeg_tiles.npz"))
    out = [(name, a, q, data, z["dec_" + name]) for name, a, q, data in tiles]
    for i in range(len(EXTRA_CASES)):
        n = "extra%d" % i
        out.append((n, z["in_" + n], int(z["q_" + n]), z["file_" + n].tobytes(), z["dec_" + n]))
    return out


# ---- files that must be refused, and variants that must decode ----------------------------

def _segment(marker, payload):
    return bytes([0xFF, marker, (len(payload) + 2) >> 8, (len(payload) + 2) & 255]) + payload


def good_variants(data):
    """[(name, bytes)]: ``data`` (a file of jpeg_literal's layout) rewritten
    with segments a decoder must tolerate; each decodes to the same picture."""
    f = bytes(data)
    dht = f[102 + 4:135] + f[135 + 4:318]      # the two tables' payloads
    return [
        ("comment_and_app1", f[:20] + _segment(0xFE, b"a comment \xFF\xD9") +
         _segment(0xE1, b"Exif\0\0" + bytes(30)) + f[20:]),
        ("dri_zero", f[:89] + _segment(0xDD, b"\0\0") + f[89:]),
        ("one_dht_segment", f[:102] + _segment(0xC4, dht) + f[318:]),
        ("second_dqt_unused", f[:89] + _segment(0xDB, bytes([1]) + bytes([7] * 64)) + f[89:]),
        ("bytes_after_eoi", f + b"\0\xFF\xD8trailing"),
    ]


def status_cases(data, pillow_files):
    """[(name, bytes, status)] built from ``data`` (a file of jpeg_literal's
    layout whose scan is longer than 40 bytes) and the bad_* files of
    jpeg_decoded.npz.  The statuses are the issue's, not any decoder's."""
    f = bytes(data)
    n = len(f)
    assert n > jl.HEADER_BYTES + 40
    cuts = [0, 1, 3, 10, 60, 95, 120, 200, jl.HEADER_BYTES, (jl.HEADER_BYTES + n) // 2, n - 3, n - 1]
    out = [("cut_%d" % c, f[:c], CORRUPT) for c in cuts]
    for name in ("progressive", "rgb", "optimised", "wide257"):
        out.append((name, bytes(pillow_files[name]), UNSUPPORTED))
    mid = jl.HEADER_BYTES + 8
    out.append(("restart_markers", f[:mid] + b"\xFF\xD0" * 5 + f[mid + 10:], CORRUPT))
    out.append(("sof1", f[:90] + b"\xC1" + f[91:], UNSUPPORTED))
    out.append(("dri_nonzero", f[:89] + _segment(0xDD, b"\0\x04") + f[89:], UNSUPPORTED))
    out.append(("dqt_16bit", f[:20] + _segment(0xDB, bytes([0x10]) + bytes([0, 3] * 64)) + f[89:],
                UNSUPPORTED))
    out.append(("no_dqt", f[:20] + f[89:], UNSUPPORTED))
    out.append(("other_huffman", f[:156] + bytes([f[157], f[156]]) + f[158:], UNSUPPORTED))
    out.append(("not_a_jpeg", b"GIF89a" + bytes(40), CORRUPT))
    out.append(("segment_past_end", f[:20] + b"\xFF\xFE\xFF\xFF" + f[20:], CORRUPT))
    out.append(("scan_all_ones", f[:jl.HEADER_BYTES] + b"\xFF\x00" * 64 + b"\xFF\xD9", CORRUPT))
    out.append(("extra_bytes_before_eoi", f[:-2] + b"\x12\x34\xFF\xD9", CORRUPT))
    return out
