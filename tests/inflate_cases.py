"""Hand-built zlib streams for the inflate tests (CPU: test_inflate_host.py,
GPU: test_gpu_inflate.py).  numpy and the standard library only.

zlib's encoder emits a small part of what RFC 1950/1951 allow, so the streams
here are written bit by bit: a deflate writer (stream-order bit packing,
canonical codes from a length list, fixed / dynamic / stored blocks, zlib
header and Adler-32 trailer) encodes a token list -- literals and (length,
distance) pairs -- and the expected bytes come from replaying the tokens.
Every valid case is checked against ``zlib.decompress`` when the families are
built (zlib is the oracle: a case it does not confirm is a bug in the writer),
and every invalid case whose fault lies in the stream's bytes is checked to
make zlib raise.

Families, each a list of Case (name, raw, stream, status, ...):
  A  format corners (valid)
  B  the match resolver's dependency patterns (valid, fixed Huffman)
  C  one stream per status clause of the decoder (invalid, exact TMH_Z_* code)
  D  every single-bit flip and truncation of four short seeds, outcome from zlib
  E  layout: offsets, alignments, launch sizes (built by the tests from A, C, D)
"""
import functools
import zlib
from typing import NamedTuple

import numpy as np

Z_OK, Z_HEADER, Z_BLOCKTYPE, Z_CODE, Z_DIST, Z_OVERFLOW = 0, 1, 2, 3, 4, 5
Z_INPUT, Z_ADLER, Z_SIZE, Z_STORED, Z_TABLE = 6, 7, 8, 9, 10
NONZERO = -1  # expected status: any error (family D: zlib decides only accept / reject)
ZCHUNK_STORED = 1
SENTINEL = 0xA5  # fill of the output buffer: bytes no chunk owns keep it


class Case(NamedTuple):
    name: str
    raw: bytes      # status 0: the decoded bytes; else the most a decoder may have written
    stream: bytes
    status: int
    raw_len: int = -1   # the table's raw_len when it is not len(raw)
    flags: int = 0
    tail: bytes = b""   # bytes after the stream in the buffer, outside src_len
    src_len: int = -1   # the table's src_len when it is not len(stream)
    in_bytes: bool = False  # invalid, and the fault lies in the stream's bytes: zlib raises too

    @property
    def n_raw(self):
        return len(self.raw) if self.raw_len < 0 else self.raw_len


# RFC 1951 3.2.5
LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99,
            115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025,
             1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0] + [e for e in range(1, 14) for _ in (0, 1)]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_L = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8  # 288 codes: 286 and 287 exist, and are invalid
FIXED_D = [5] * 32
# a complete code over all 19 code-length symbols: 13/16 + 6/32 = 1
CL_ALL = [4] * 13 + [5] * 6


class BitWriter:
    """Bits in stream order (RFC 1951 3.1.1: least significant bit of a byte first)."""

    def __init__(self):
        self.parts, self.acc, self.n, self.total = [], 0, 0, 0

    def put(self, v, n):
        self.acc |= (v & ((1 << n) - 1)) << self.n
        self.n += n
        if self.n >= 4096:
            self._spill()

    def _spill(self):
        if self.n:
            b = np.frombuffer(self.acc.to_bytes((self.n + 7) // 8, "little"), np.uint8)
            self.parts.append(np.unpackbits(b, bitorder="little")[:self.n])
            self.total += self.n
            self.acc = self.n = 0

    def put_array(self, bits):
        self._spill()
        self.parts.append(bits)
        self.total += len(bits)

    def put_bytes(self, data):
        assert (self.total + self.n) % 8 == 0
        self.put_array(np.unpackbits(np.frombuffer(data, np.uint8), bitorder="little"))

    def align(self):
        self.put(0, -(self.total + self.n) % 8)

    def nbits(self):
        return self.total + self.n

    def tobytes(self):
        self._spill()
        if not self.parts:
            return b""
        return np.packbits(np.concatenate(self.parts), bitorder="little").tobytes()


def _rev(code, n):
    return int(format(code, "0%db" % n)[::-1], 2) if n else 0


class Code:
    """Canonical Huffman code of a length list (RFC 1951 3.2.2), each code
    bit-reversed so that it goes into the stream with one put()."""

    def __init__(self, lens):
        self.lens = list(lens)
        count = [0] * 17
        for l in self.lens:
            count[l] += 1
        count[0] = 0
        nxt, code = [0] * 17, 0
        for l in range(1, 17):
            code = (code + count[l - 1]) << 1
            nxt[l] = code
        self.rev = [0] * len(self.lens)
        for s, l in enumerate(self.lens):
            if l:
                self.rev[s] = _rev(nxt[l] & ((1 << l) - 1), l)
                nxt[l] += 1
        self._rev_a = np.array(self.rev[:256] + [0] * max(0, 256 - len(self.rev)), np.uint32)
        self._len_a = np.array(self.lens[:256] + [0] * max(0, 256 - len(self.lens)), np.int64)

    def put(self, w, s):
        assert self.lens[s], "symbol %d has no code" % s
        w.put(self.rev[s], self.lens[s])

    def put_literals(self, w, data):
        """A run of literal bytes, vectorised."""
        a = np.frombuffer(data, np.uint8)
        l = self._len_a[a]
        assert l.all()
        k = np.arange(15)
        bits = ((self._rev_a[a][:, None] >> k) & 1).astype(np.uint8)
        w.put_array(bits[k < l[:, None]])


def kraft(lens):
    """Sum of 2^-l over the codes, in units of 2^-15 (complete: 32768)."""
    return sum(1 << (15 - l) for l in lens if l)


def flat_lens(n):
    """A complete code over n >= 2 symbols with lengths k and k + 1."""
    k = n.bit_length() - 1
    x = (2 << k) - n
    return [k] * x + [k + 1] * (n - x)


def len_symbol(length):
    s = max(i for i in range(29) if LEN_BASE[i] <= length)
    return s, length - LEN_BASE[s]


def dist_symbol(dist):
    s = max(i for i in range(30) if DIST_BASE[i] <= dist)
    return s, dist - DIST_BASE[s]


def replay(tokens):
    """The bytes a token list decodes to."""
    out = bytearray()
    for t in tokens:
        if isinstance(t, int):
            out.append(t)
        elif isinstance(t, (bytes, bytearray)):
            out += t
        elif isinstance(t[0], int):
            length, dist = t[0], t[1]
            assert 1 <= dist <= len(out)
            if dist >= length:
                out += out[len(out) - dist:len(out) - dist + length]
            else:
                for _ in range(length):
                    out.append(out[-dist])
    return bytes(out)


def put_tokens(w, tokens, lcode, dcode, eob=True):
    """Tokens: an int (literal), bytes (a literal run), (length, distance) or
    (length, distance, length symbol index) for a chosen length symbol; and,
    for invalid streams, ("lsym", s) / ("dsym", s) / ("raw", value, bits)."""
    for t in tokens:
        if isinstance(t, int):
            lcode.put(w, t)
        elif isinstance(t, (bytes, bytearray)):
            if len(t) < 16:
                for x in t:
                    lcode.put(w, x)
            else:
                lcode.put_literals(w, bytes(t))
        elif t[0] == "lsym":
            lcode.put(w, t[1])
        elif t[0] == "dsym":
            dcode.put(w, t[1])
        elif t[0] == "raw":
            w.put(t[1], t[2])
        else:
            ls, lx = len_symbol(t[0]) if len(t) < 3 else (t[2], t[0] - LEN_BASE[t[2]])
            assert 0 <= lx < (1 << LEN_EXTRA[ls]) or (LEN_EXTRA[ls] == 0 and lx == 0)
            lcode.put(w, 257 + ls)
            w.put(lx, LEN_EXTRA[ls])
            ds, dx = dist_symbol(t[1])
            dcode.put(w, ds)
            w.put(dx, DIST_EXTRA[ds])
    if eob:
        lcode.put(w, 256)


def rle_lengths(lens):
    """The code lengths as code-length symbols with the repeat codes 16/17/18:
    [(symbol, extra value)], runs taken over the whole list (so they cross
    from the literal/length into the distance lengths, which zlib's encoder
    never does)."""
    seq, i = [], 0
    while i < len(lens):
        v, c = lens[i], 1
        while i + c < len(lens) and lens[i + c] == v:
            c += 1
        i += c
        if v:
            seq.append((v, 0))
            c -= 1
        while not v and c >= 11:
            r = min(c, 138)
            seq.append((18, r - 11))
            c -= r
        while c >= 3:
            r = min(c, 10 if not v else 6)
            seq.append((17 if not v else 16, r - 3))
            c -= r
        seq += [(v, 0)] * c
    return seq


CL_EXTRA = {16: 2, 17: 3, 18: 7}


def put_dynamic_header(w, final, llens, dlens, cl_lens=None, hclen=19, repeat=True, cl_seq=None,
                       hlit=None, hdist=None):
    """BFINAL, BTYPE = 2, HLIT, HDIST, HCLEN, the code-length code's lengths
    (the first hclen of CL_ORDER) and the two codes' lengths, sent through
    the code-length code: cl_seq, or the lengths run-length coded (repeat) or
    one symbol per length."""
    cl_lens = CL_ALL if cl_lens is None else cl_lens
    w.put(final, 1)
    w.put(2, 2)
    w.put((len(llens) if hlit is None else hlit) - 257, 5)
    w.put((len(dlens) if hdist is None else hdist) - 1, 5)
    w.put(hclen - 4, 4)
    for i in range(hclen):
        w.put(cl_lens[CL_ORDER[i]], 3)
    assert not any(cl_lens[s] for s in CL_ORDER[hclen:])
    if cl_seq is None:
        both = list(llens) + list(dlens)
        cl_seq = rle_lengths(both) if repeat else [(v, 0) for v in both]
    cl = Code(cl_lens)
    for s, x in cl_seq:
        cl.put(w, s)
        w.put(x, CL_EXTRA.get(s, 0))


def put_stored(w, final, data, nlen=None):
    w.put(final, 1)
    w.put(0, 2)
    w.align()
    w.put(len(data), 16)
    w.put((len(data) ^ 0xFFFF) if nlen is None else nlen, 16)
    if data:
        w._spill()
        w.put_bytes(data)


def put_fixed(w, final, tokens, eob=True):
    w.put(final, 1)
    w.put(1, 2)
    put_tokens(w, tokens, _FIXED_LC, _FIXED_DC, eob)


def put_dynamic(w, final, tokens, llens, dlens, eob=True, **kw):
    put_dynamic_header(w, final, llens, dlens, **kw)
    put_tokens(w, tokens, Code(llens), Code(dlens), eob)


_FIXED_LC, _FIXED_DC = Code(FIXED_L), Code(FIXED_D)


def seal(w, raw, header=b"\x78\x9c", adler=None):
    """The zlib stream: header, the writer's deflate blocks, Adler-32 of raw."""
    w.align()
    a = zlib.adler32(raw) if adler is None else adler
    return header + w.tobytes() + a.to_bytes(4, "big")


def fixed_stream(tokens):
    w = BitWriter()
    put_fixed(w, 1, tokens)
    return seal(w, replay(tokens))


def _valid(name, tokens_or_raw, stream, **kw):
    raw = tokens_or_raw if isinstance(tokens_or_raw, bytes) else replay(tokens_or_raw)
    return Case(name, raw, stream, Z_OK, **kw)


def _rand(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def _lit_code(extra_syms=()):
    """A complete literal/length code: every literal byte, the end-of-block
    code and the given length symbols."""
    syms = list(range(257)) + [257 + s for s in extra_syms]
    lens = [0] * (max(syms) + 1)
    for s, l in zip(syms, flat_lens(len(syms))):
        lens[s] = l
    return lens


def _codes_for(tokens):
    """Complete codes holding just what the tokens use."""
    ls = sorted({len_symbol(t[0])[0] if len(t) < 3 else t[2] for t in tokens
                 if isinstance(t, tuple) and isinstance(t[0], int)})
    ds = sorted({dist_symbol(t[1])[0] for t in tokens
                 if isinstance(t, tuple) and isinstance(t[0], int)})
    return _lit_code(ls), (_dist_code(ds) if ds else [0])


def _dist_code(syms):
    lens = [0] * (max(syms) + 1)
    if len(syms) == 1:
        lens[syms[0]] = 1
    else:
        for s, l in zip(syms, flat_lens(len(syms))):
            lens[s] = l
    return lens


# ---------------------------------------------------------------- family A

def family_a():
    out = []

    def dyn(name, tokens, llens, dlens, **kw):
        w = BitWriter()
        put_dynamic(w, 1, tokens, llens, dlens, **kw)
        out.append(_valid(name, tokens, seal(w, replay(tokens))))

    # distance 32768 (symbol 29, all 13 extra bits set) at the 8-byte copy group's edges
    far = _rand(32768, 11)
    for length in (3, 4, 8, 9, 257, 258):
        out.append(_valid("dist32768_len%d" % length, [far, (length, 32768)],
                          fixed_stream([far, (length, 32768)])))
    # the same through a dynamic block whose distance code holds only symbols 28 and 29
    toks = [far, (258, 32768), (3, 16385), (7, 24576), (9, 24577)]
    dyn("dist32768_dynamic", toks, *_codes_for(toks))
    assert _codes_for(toks)[1] == [0] * 28 + [1, 1]
    # every distance symbol at its smallest and largest extra bits; every length symbol too
    pre = _rand(32768, 12)
    toks = [pre]
    for s in range(30):
        toks += [(3 + s % 7, DIST_BASE[s]), 65 + s, (4, DIST_BASE[s] + (1 << DIST_EXTRA[s]) - 1)]
    out.append(_valid("every_dist_symbol_fixed", toks, fixed_stream(toks)))
    dyn("every_dist_symbol_dynamic", toks, _lit_code(range(8)), flat_lens(30))
    toks = [_rand(300, 13)]
    for s in range(29):
        toks += [(LEN_BASE[s], 1 + 9 * s), s,
                 (LEN_BASE[s] + (1 << LEN_EXTRA[s]) - 1, 300 - s, s)]
    assert (258, 273, 27) in toks  # 258 through symbol 284 and 31 extra, next to symbol 285's
    out.append(_valid("every_len_symbol_fixed", toks, fixed_stream(toks)))
    dyn("every_len_symbol_dynamic", toks, _lit_code(range(29)), flat_lens(30))
    dyn("every_len_symbol_plain_lengths", toks, _lit_code(range(29)), flat_lens(30), repeat=False)
    # codes of every length 1..15: literals 0..13 = 1..14 bits, end-of-block and
    # length symbol 257 = 15 bits; distance symbols 0..15 likewise
    ladder = list(range(1, 16)) + [15]
    ll = [0] * 258
    for s, l in zip(list(range(14)) + [256, 257], ladder):
        ll[s] = l
    toks = list(range(14)) * 16 + [(3, d) for d in (1, 2, 3, 4, 5, 7, 9, 13, 17, 25)] + \
        [13, 12, 13, (3, 33), (3, 49), (3, 65), (3, 97), (3, 129), (3, 193), 11, 13]
    dyn("ladder_1_to_15", toks, ll, ladder)
    # chains of 15-bit codes (the canonical search, not the first-level table):
    # lengths 1..8 once each and 128 codes of 15 bits
    ll = [0] * 258
    for s in range(128):
        ll[s] = 15
    for i, s in enumerate([256, 257] + list(range(128, 134))):
        ll[s] = 1 + i
    assert kraft(ll) == 32768
    dd = [15] * 16 + list(range(11, 0, -1))
    assert kraft(dd) == 32768
    toks = [bytes(range(128)) * 3] + [(3, DIST_BASE[s]) for s in range(16)] + [bytes(range(127, 0, -3))]
    dyn("chains_of_15_bit_codes", toks, ll, dd)
    # HCLEN: 19 above (CL_ALL); here the field value 4, i.e. the eight lengths of
    # 16, 17, 18, 0, 8, 7, 9, 6.  (Field value 0 -- four lengths -- can only spell
    # zeros, so no end-of-block code: family C.)
    cl8 = [0] * 19
    cl8[8], cl8[16], cl8[9], cl8[0] = 1, 2, 3, 3
    dyn("hclen_8_lengths", [_rand(200, 14)],
        [8] * 255 + [9, 9], [0], cl_lens=cl8, hclen=8)
    # repeat codes running from the literal/length lengths into the distance lengths
    ll = [8] * 191 + [0] * 65 + [8] + [4] * 4
    lits = bytes(np.frombuffer(_rand(150, 15), np.uint8) % 191)
    dyn("repeat16_crosses", [lits, (3, 1), (5, 9), (6, 150)], ll, [4] * 16)
    seq = rle_lengths(ll + [4] * 16)
    assert seq[-4:] == [(16, 3)] * 3 + [(4, 0)] and len(ll) == 261
    ll = _lit_code() + [0, 0]
    dyn("repeat17_crosses", [lits, 255], ll, [0, 0, 0, 0, 1])
    assert (17, 3) in rle_lengths(ll + [0, 0, 0, 0, 1])
    ll = _lit_code((0, 1)) + [0] * 20
    dyn("repeat18_crosses", [lits, (3, 150), (4, 128), (3, 96), (4, 66)], ll, [0] * 12 + [2] * 4)
    assert (18, 32 - 11) in rle_lengths(ll + [0] * 12 + [2] * 4)
    # the incomplete codes zlib allows
    toks = [7, 8, (200, 1), 9, (3, 1)]
    dyn("one_distance_code_length_1", toks, _codes_for(toks)[0], [1])
    dyn("no_distance_code", [lits], _lit_code(), [0])
    dyn("end_of_block_only_literal_code", [], [0] * 256 + [1], [0])
    w = BitWriter()
    put_dynamic(w, 0, [], [0] * 256 + [1], [0])
    put_fixed(w, 1, [lits])
    out.append(_valid("end_of_block_only_then_data", lits, seal(w, lits)))
    # empty blocks
    out.append(_valid("empty_fixed", b"", fixed_stream([])))
    dyn("empty_dynamic", [], _lit_code(), [0])
    w = BitWriter()
    put_stored(w, 1, b"")
    out.append(_valid("empty_stored", b"", seal(w, b"")))
    w = BitWriter()
    for i in range(300):
        if i % 3 == 0:
            put_fixed(w, 0, [])
        elif i % 3 == 1:
            put_stored(w, 0, b"")
        else:
            put_dynamic(w, 0, [], [0] * 256 + [1], [0])
    put_fixed(w, 1, [lits, (30, 150)])
    out.append(_valid("300_empty_blocks_first", [lits, (30, 150)], seal(w, replay([lits, (30, 150)]))))
    # stored blocks: 0 and 65535 bytes, and one after a block ending inside a byte
    big = _rand(65535, 16)
    w = BitWriter()
    put_stored(w, 0, b"")
    put_stored(w, 0, big)
    put_stored(w, 1, b"")
    out.append(_valid("stored_0_65535_0", big, seal(w, big)))
    ends = set()
    for k in range(8):  # 9-bit literals: the fixed block ends at every bit position of a byte
        head = [bytes([200]) * k + lits[:1], (3, 1)]
        w = BitWriter()
        put_fixed(w, 0, head)
        ends.add(w.nbits() % 8)
        put_stored(w, 0, lits)
        put_fixed(w, 1, [(9, 150), 66])
        raw = replay(head + [lits, (9, 150), 66])
        out.append(_valid("stored_after_%d_nine_bit_literals" % k, raw, seal(w, raw)))
    assert ends == set(range(8))
    # bytes after the trailer, inside src_len: zlib ignores them (unused_data)
    s = fixed_stream([lits, (20, 75)])
    out.append(_valid("data_after_trailer", [lits, (20, 75)], s + _rand(37, 17)))
    for c in out:
        d = zlib.decompressobj()
        assert d.decompress(c.stream) == c.raw and d.eof, c.name
    assert len({c.name for c in out}) == len(out)
    return out


# ---------------------------------------------------------------- family B

def _b_matrix():
    """Every length 3..258 with the distances where the resolver's copy changes
    form: distance >= length (8-byte groups) or below it (byte by byte)."""
    out = []
    pre = _rand(260, 21)
    for length in range(3, 259):
        for dist in sorted({1, 2, 3, 4, 7, 8, 9, length - 1, length, length + 1}):
            toks = [pre[:dist + (length + dist) % 3], (length, dist), 33]
            out.append(_valid("m_len%d_dist%d" % (length, dist), toks, fixed_stream(toks)))
    return out


def _b_random(n_streams=300):
    """Token streams of 63, 64, 65, 128 or 129 matches (the resolver takes 64
    per batch).  Every match's source is placed against an earlier match's
    destination [o_k, o_k + len_k): ending exactly at the previous one's start
    (may copy in the same round), one byte inside it (must wait), inside the
    destination 63 or 64 matches back (the batch edge), or in the literal
    prefix alone."""
    rng = np.random.default_rng(22)
    out = []
    for si in range(n_streams):
        n_match = (63, 64, 65, 128, 129)[si % 5]
        prefix = rng.integers(0, 256, int(rng.integers(260, 300)), dtype=np.uint8).tobytes()
        toks, o, dests, modes = [prefix], len(prefix), [], [0, 0, 0, 0]
        while len(dests) < n_match:
            for _ in range(int(rng.integers(0, 3))):  # 0..2 literals between matches
                toks.append(int(rng.integers(0, 256)))
                o += 1
            length = int(rng.integers(3, 24)) if rng.random() < 0.9 else int(rng.integers(24, 259))
            mode = int(rng.integers(0, 4)) if dests else 3
            m = len(dests)
            if mode == 0:    # src_end == o_prev
                dist = o - dests[-1][0] + length
            elif mode == 1:  # src_end == o_prev + 1
                dist = o - dests[-1][0] + length - 1
            elif mode == 2 and m >= 63:
                ok, lk = dests[m - (64 if m >= 64 and rng.random() < 0.5 else 63)]
                dist = o - (ok + int(rng.integers(1, lk + 1))) + length
            else:
                mode = 3
                dist = o - int(rng.integers(0, len(prefix) - length + 1))
            if not (length <= dist <= min(o, 32768)):
                mode = 3
                dist = o - int(rng.integers(0, len(prefix) - length + 1))
            assert 1 <= dist <= min(o, 32768)
            modes[mode] += 1
            toks.append((length, dist))
            dests.append((o, length))
            o += length
        assert min(modes[:2]) > 5 and modes[3] > 0 and (n_match < 128 or modes[2] > 3), modes
        out.append(_valid("r%d_%dmatches" % (si, n_match), toks, fixed_stream(toks)))
    return out


def _b_capacity():
    """The longest match list a chunk of raw_len bytes can have: one literal,
    then matches of 3 bytes (and the literals that fill up raw_len)."""
    out = []
    for n in (4, 7, 3001, 3002, 3003):
        toks = [90] + [(3, 1)] * ((n - 1) // 3) + [91] * ((n - 1) % 3)
        out.append(_valid("cap_%d" % n, toks, fixed_stream(toks)))
        assert len(out[-1].raw) == n
    return out


def family_b():
    out = _b_matrix() + _b_random() + _b_capacity()
    for c in out:
        assert zlib.decompress(c.stream) == c.raw, c.name
    return out


# ---------------------------------------------------------------- family C

def family_c():
    out = []
    lits = bytes(np.frombuffer(_rand(150, 31), np.uint8) % 191)
    good_toks = [lits, (20, 75), 5, (258, 1)]
    good_raw = replay(good_toks)
    good = fixed_stream(good_toks)
    w = BitWriter()
    put_fixed(w, 1, good_toks)
    body = w.tobytes()

    def add(name, status, stream, written=b"", in_bytes=True, **kw):
        out.append(Case(name, written, stream, status, in_bytes=in_bytes, **kw))

    def fixed(name, status, tokens, written, eob=True, **kw):
        w = BitWriter()
        put_fixed(w, 1, tokens, eob)
        w.put(0, 64)  # zero bits behind the fault, so the decoder is not short of input
        add(name, status, seal(w, written), written, raw_len=kw.pop("raw_len", len(written) + 600),
            **kw)

    def dyn(name, status, tokens, llens, dlens, written=b"", **kw):
        w = BitWriter()
        put_dynamic(w, 1, tokens, llens, dlens, **kw)
        w.put(0, 64)
        add(name, status, seal(w, written), written, raw_len=len(written) + 600)

    # 1: the zlib header
    tr = zlib.adler32(good_raw).to_bytes(4, "big")
    assert 0x7785 % 31 == 0 and 0x8898 % 31 == 0 and 0x7820 % 31 == 0
    add("header_cm_7", Z_HEADER, b"\x77\x85" + body + tr, raw_len=len(good_raw))
    add("header_cinfo_8", Z_HEADER, b"\x88\x98" + body + tr, raw_len=len(good_raw))
    add("header_fcheck", Z_HEADER, b"\x78\x9d" + body + tr, raw_len=len(good_raw))
    add("header_fdict", Z_HEADER, b"\x78\x20" + body + tr, raw_len=len(good_raw))
    # 2: block type 3
    w = BitWriter()
    put_fixed(w, 0, [lits])
    w.put(1, 1)
    w.put(3, 2)
    w.put(0, 64)
    add("block_type_3", Z_BLOCKTYPE, seal(w, lits), lits, raw_len=len(lits) + 600)
    # 3: symbols the code has no meaning or no code for
    for s in (286, 287):
        fixed("length_symbol_%d" % s, Z_CODE, [lits, ("lsym", s)], lits, eob=False)
    for s in (30, 31):
        fixed("distance_symbol_%d" % s, Z_CODE, [lits, ("lsym", 257), ("dsym", s)], lits, eob=False)
    # one distance code of 1 bit (0): the bit 1 is a pattern the code does not hold
    dyn("pattern_not_in_distance_code", Z_CODE, [lits, ("lsym", 257), ("raw", 1, 1)],
        _lit_code((0,)), [1], lits, eob=False)
    # 4: a distance one past the bytes so far
    fixed("distance_past_start", Z_DIST, [lits, (3, len(lits) + 1)], lits, eob=False)
    fixed("distance_at_first_byte", Z_DIST, [(3, 1)], b"", eob=False)
    # 5: one byte more than raw_len, by a literal, a match and a stored byte
    add("overflow_literal", Z_OVERFLOW, fixed_stream([lits, (20, 75), 5]), replay([lits, (20, 75)]),
        raw_len=170, in_bytes=False)
    add("overflow_match", Z_OVERFLOW, fixed_stream([lits, (20, 75)]), lits, raw_len=169, in_bytes=False)
    w = BitWriter()
    put_stored(w, 1, lits)
    add("overflow_stored", Z_OVERFLOW, seal(w, lits), lits[:149], raw_len=149, in_bytes=False)
    # 6: the stream's last byte lies outside src_len (the next bytes of the
    # buffer happen to complete it); a table entry past the buffer's end
    add("input_borrowed_trailer_byte", Z_INPUT, good[:-1], good_raw, tail=good[-1:])
    add("input_entry_past_buffer", Z_INPUT, good, b"", raw_len=len(good_raw), src_len=1 << 40,
        in_bytes=False)
    # 7, 8
    add("adler_mismatch", Z_ADLER, good[:-1] + bytes([good[-1] ^ 0x80]), good_raw)
    add("size_one_short", Z_SIZE, good, good_raw, raw_len=len(good_raw) + 1, in_bytes=False)
    # 9
    w = BitWriter()
    put_fixed(w, 0, [lits])
    put_stored(w, 1, lits, nlen=(len(lits) ^ 0xFFFF) ^ 0x0100)
    add("stored_len_nlen", Z_STORED, seal(w, lits + lits), lits, raw_len=2 * len(lits))
    # 10: code lengths no code can have
    base_l = _lit_code((0,))
    dyn("table_oversubscribed_literals", Z_TABLE, [], [8] * 257 + [1], [0])
    dyn("table_oversubscribed_distances", Z_TABLE, [], base_l, [1, 1, 1])
    cl = [0] * 19
    cl[0], cl[8], cl[9] = 1, 1, 1
    dyn("table_oversubscribed_code_lengths", Z_TABLE, [], [8] * 255 + [9, 9], [0], cl_lens=cl,
        repeat=False)
    dyn("table_no_end_of_block", Z_TABLE, [], [8] * 255 + [9, 0, 9], [0], eob=False)
    cl4 = [0] * 19
    cl4[0], cl4[18] = 1, 1
    dyn("table_hclen_4_lengths_spell_only_zeros", Z_TABLE, [], [0] * 257, [0], cl_lens=cl4, hclen=4,
        eob=False)
    dyn("table_repeat_16_first", Z_TABLE, [], base_l, [0], cl_seq=[(16, 0)] + rle_lengths(base_l),
        eob=False)
    dyn("table_repeat_past_end", Z_TABLE, [], base_l, [0],
        cl_seq=rle_lengths(base_l) + [(18, 0)], eob=False)
    dyn("table_repeat_16_past_end", Z_TABLE, [], base_l, [5, 5],
        cl_seq=rle_lengths(base_l) + [(5, 0), (16, 0)], eob=False)
    dyn("table_hlit_287", Z_TABLE, [], base_l, [0], hlit=287, eob=False)
    dyn("table_hlit_288", Z_TABLE, [], base_l, [0], hlit=288, eob=False)
    dyn("table_hdist_31", Z_TABLE, [], base_l, [0], hdist=31, eob=False)
    dyn("table_hdist_32", Z_TABLE, [], base_l, [0], hdist=32, eob=False)
    out += incomplete_codes()
    for c in out:
        if c.in_bytes:
            try:
                zlib.decompress(c.stream)
            except zlib.error:
                continue
            raise AssertionError("zlib accepts " + c.name)
    assert len({c.name for c in out}) == len(out)
    return out


def incomplete_codes():
    """Streams whose tokens decode, with a correct Adler-32, but whose code
    lengths zlib's inflate_table rejects as an incomplete set: allowed only
    as exactly one code of length 1 (or, for distances, none), and never for
    the code-length code."""
    out = []
    lits = bytes(np.frombuffer(_rand(150, 32), np.uint8) % 100)

    def dyn(name, tokens, llens, dlens, **kw):
        w = BitWriter()
        put_dynamic(w, 1, tokens, llens, dlens, **kw)
        raw = replay(tokens)
        out.append(Case(name, b"", seal(w, raw), Z_TABLE, raw_len=len(raw), in_bytes=True))

    toks = [lits, (20, 75), 5, (3, 2)]
    full = _lit_code((0, 12))
    short = list(full)
    short[255] = 0  # one code fewer: incomplete
    assert kraft(full) == 32768 and kraft(short) < 32768
    dyn("incomplete_literal_code", toks, short, [2, 2] + [0] * 9 + [2, 2])
    dyn("incomplete_distance_code", toks, full, [2, 2] + [0] * 10 + [2])
    dyn("one_distance_code_length_2", [lits, (20, 1), 5, (3, 1)], full, [2])
    dyn("two_literal_codes_length_2", [], [0] * 255 + [2, 2], [0])
    dyn("one_literal_code_length_2", [], [0] * 256 + [2], [0])
    cl = [0] * 19
    cl[0], cl[8], cl[9], cl[18] = 2, 2, 3, 3  # 3/4: incomplete
    dyn("incomplete_code_length_code", [lits], [8] * 255 + [9, 9], [0], cl_lens=cl, repeat=False)
    cl = [0] * 19
    cl[0] = 1  # a single code: every length 0 (also no end-of-block code)
    w = BitWriter()
    put_dynamic_header(w, 1, [0] * 257, [0], cl_lens=cl, repeat=False)
    w.put(0, 64)
    out.append(Case("single_code_length_code", b"", seal(w, b""), Z_TABLE, raw_len=100, in_bytes=True))
    return out


# ---------------------------------------------------------------- family D

def seeds():
    """Four short streams: dynamic, fixed, stored, and two blocks with a sync flush."""
    text = (b"site %d of well D%02d, channel %s: illumination statistics; " * 5) % (
        3, 4, b"DAPI", 4, 4, b"GFP", 5, 5, b"Cy5", 6, 6, b"DAPI", 7, 7, b"GFP")
    rng = np.random.default_rng(41)
    words = (rng.integers(0, 30, 260) * 7 % 97 + 32).astype(np.uint8).tobytes()
    out = [("dynamic", text + words, zlib.compress(text + words, 9))]
    co = zlib.compressobj(9, zlib.DEFLATED, 15, 8, zlib.Z_FIXED)
    out.append(("fixed", text, co.compress(text) + co.flush()))
    out.append(("stored", words[:120], zlib.compress(words[:120], 0)))
    co = zlib.compressobj(6)
    s = co.compress(text[:150]) + co.flush(zlib.Z_SYNC_FLUSH) + co.compress(text[150:] + words[:60])
    out.append(("two_blocks", text + words[:60], s + co.flush()))
    for name, raw, s in out:
        assert 100 <= len(s) <= 400 and zlib.decompress(s) == raw, (name, len(s))
    return out


def _zlib_outcome(stream):
    """(bytes, None) when zlib inflates the stream to its end, else (None, error)."""
    d = zlib.decompressobj()
    try:
        got = d.decompress(stream)
    except zlib.error as e:
        return None, e
    return (got, None) if d.eof else (None, "incomplete")


def family_d():
    out = []
    for sname, raw, s in seeds():
        muts = [("%s_flip_%d_%d" % (sname, i, b), s[:i] + bytes([s[i] ^ (1 << b)]) + s[i + 1:],
                 i >= 2) for i in range(len(s)) for b in range(8)]
        muts += [("%s_cut_%d" % (sname, n), s[:n], False) for n in range(len(s))]
        for name, m, reseal in muts:
            got, _ = _zlib_outcome(m)
            if got is not None and len(got) == len(raw):
                out.append(Case(name, got, m, Z_OK))
            else:  # zlib raises, stops short of the end, or gives another length
                out.append(Case(name, b"", m, NONZERO, raw_len=len(raw)))
            if not reseal:  # truncations, and flips in the zlib header
                continue
            # the flipped deflate data alone, when it still is a deflate stream:
            # resealed with its own Adler-32, cut at its own end
            d = zlib.decompressobj(-15)
            try:
                got = d.decompress(m[2:])
            except zlib.error:
                continue
            if d.eof:
                end = len(m) - 2 - len(d.unused_data)
                re = s[:2] + m[2:2 + end] + zlib.adler32(got).to_bytes(4, "big")
                assert zlib.decompress(re) == got
                out.append(Case(name + "_resealed", got, re, Z_OK))
    return out


# ---------------------------------------------------------------- layout

@functools.lru_cache(maxsize=None)
def families():
    return {"A": family_a(), "B": family_b(), "C": family_c(), "D": family_d()}


def family_e():
    """Layout: [(name, cases, layout arguments)], one launch each."""
    fam = families()
    by_name = {c.name: c for c in fam["A"]}
    one = by_name["repeat16_crosses"]  # a dynamic block, literals and matches, under 300 bytes
    jobs = [("off_src%d_out%d_trail%d" % (so, ro, tr), [one],
             dict(src_lead=so, raw_lead=ro, src_trail=tr, gaps=False, raw_trail=2))
            for so in range(40) for ro in (0, 1, 5, 15) for tr in (0, 1, 15, 16, 17)]
    # launches of 1, W - 1, W and W + 1 streams for the workgroup widths 4, 8 and 64
    small = [c for c in fam["A"] if c.n_raw < 2000]
    for n in (1, 3, 4, 5, 7, 8, 9, 63, 64, 65):
        jobs.append(("launch_of_%d" % n, [small[(i * 7 + n) % len(small)] for i in range(n)], {}))
    # failing, short and long streams side by side in the workgroups
    mixed = []
    for i in range(len(fam["A"])):
        mixed += [fam["A"][i], fam["C"][i % len(fam["C"])]] + fam["D"][i::len(fam["A"])][:9]
    mixed += fam["C"]
    jobs.append(("mixed_families", mixed, dict(src_lead=1)))
    # chunks whose filter was skipped (TMH_ZCHUNK_STORED) at odd offsets between deflated ones
    body = _rand(300, 51)
    st = [Case("stored_77", body[:77], body[:77], Z_OK, flags=ZCHUNK_STORED),
          Case("stored_1", body[:1], body[:1], Z_OK, flags=ZCHUNK_STORED),
          Case("stored_0", b"", b"", Z_OK, flags=ZCHUNK_STORED),
          Case("stored_short", b"", body[:50], Z_SIZE, raw_len=51, flags=ZCHUNK_STORED),
          Case("stored_long", b"", body[:52], Z_SIZE, raw_len=51, flags=ZCHUNK_STORED),
          Case("stored_zlib_bytes", one.stream, one.stream, Z_OK, flags=ZCHUNK_STORED),
          Case("stored_300", body, body, Z_OK, flags=ZCHUNK_STORED)]
    cases = []
    for i, c in enumerate(st):
        cases += [small[i], c]
    jobs.append(("stored_chunks", cases + [one], dict(src_lead=1)))
    return jobs


def layout(cases, src_lead=0, raw_lead=3, src_trail=0, gaps=True, raw_trail=None):
    """The cases as one launch: (blob, table rows, raw_bytes).  Rows are
    (src_off, src_len, raw_off, raw_len, flags).  Streams follow each other
    (each with its tail); outputs are separated by 0..2 bytes no chunk owns
    when gaps is set, so they lie at every alignment."""
    blob = bytearray(b"\xee" * src_lead)
    rows, roff = [], raw_lead
    for i, c in enumerate(cases):
        rows.append((len(blob), len(c.stream) if c.src_len < 0 else c.src_len, roff, c.n_raw,
                     c.flags))
        blob += c.stream + c.tail
        roff += c.n_raw + (i % 3 if gaps else 0)
    blob += b"\xee" * src_trail
    return bytes(blob), rows, roff + ((4 if gaps else 0) if raw_trail is None else raw_trail)


def owned_mask(rows, raw_bytes):
    m = np.zeros(raw_bytes, bool)
    for _, _, ro, rl, _ in rows:
        m[ro:ro + rl] = True
    return m


def split_launches(cases, max_words=1 << 24):
    """Consecutive groups whose match lists (cases x the longest raw_len / 3
    entries of two words) stay under max_words."""
    groups, cur, big = [], [], 0
    for c in cases:
        nb = max(big, c.n_raw)
        if cur and (len(cur) + 1) * (2 * (nb // 3) + 24) > max_words:
            groups.append(cur)
            cur, nb = [], c.n_raw
        cur.append(c)
        big = nb
    if cur:
        groups.append(cur)
    return groups


def check_outputs(cases, rows, raw_out, status, where=""):
    """The statuses and bytes one launch must give: exact status (NONZERO:
    any error), exact bytes for status 0, the sentinel beyond what a failed
    chunk may have written and in every byte no chunk owns."""
    raw_out = np.asarray(raw_out, np.uint8)
    bad = [(c.name, c.status, int(s)) for c, s in zip(cases, status)
           if (s == 0 if c.status == NONZERO else s != c.status)]
    assert not bad, "%s (name, expected, got): %s" % (where, bad[:20])
    assert np.all(raw_out[~owned_mask(rows, len(raw_out))] == SENTINEL), where + ": wrote outside the chunks"
    for c, (_, _, ro, rl, _) in zip(cases, rows):
        got = raw_out[ro:ro + rl]
        if c.status == Z_OK:
            assert got.tobytes() == c.raw, "%s %s: bytes differ" % (where, c.name)
        elif c.status != NONZERO:
            assert np.all(got[len(c.raw):] == SENTINEL), "%s %s: wrote past its fault" % (where, c.name)
