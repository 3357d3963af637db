// PNG encode of greyscale channel images: the core of png_kernels.hip, kept
// free of HIP headers so the same code builds for the host
// (tests/png_host.cpp: a workgroup of one thread, a wave of one lane).  The
// expensive part of a PNG is its zlib stream; deflate_core.h codes it, cut
// into pieces that workgroups code side by side (deflate_piece).  Here: the
// row filters, the CRC-32 of a chunk computed by all threads, the Adler-32
// joined from the pieces' sums, the chunk framing.  DESIGN §26 has the rules:
//  - colour type 0, bit depth 8 or 16 (samples big-endian), no interlace;
//  - the filtered stream is, per row, the filter type and the filtered bytes;
//    the type is the one with the smallest sum of v < 128 ? v : 256 - v over
//    the row's filtered bytes, ties to the lowest type; every filter reads
//    the raw row above, so rows are independent;
//  - the stream is cut into pieces of kPngPiece bytes, one IDAT chunk each,
//    and one last IDAT holds the Adler-32 alone, so that no chunk's CRC
//    depends on another piece.
// No result depends on the number of threads or lanes.
#pragma once

#include "deflate_core.h"

#ifndef TMH_PNG_PIECE_SEGS
#define TMH_PNG_PIECE_SEGS 1  // segments of a piece: DESIGN §26.5 has 1 against 4
#endif

#ifndef TMH_PSUM64
// a value summed over the 64 lanes that share a row (all of them arrive)
#define TMH_PSUM64(v) ::tmh::png_wave_sum(v)
namespace tmh {
namespace {
__device__ __forceinline__ uint64_t png_wave_sum(uint64_t v) {
  for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}
}  // namespace
}  // namespace tmh
#endif

namespace tmh {

namespace {

constexpr int64_t kPngPiece = (int64_t)TMH_PNG_PIECE_SEGS * kDSeg;
constexpr int kPngHead = 33;  // signature and IHDR
constexpr int kPngTail = 28;  // the Adler-32's IDAT and IEND

TMH_DHD int64_t png_row_bytes(int width, int es) { return 1 + (int64_t)width * es; }
TMH_DHD int64_t png_stream_bytes(int height, int width, int es) {
  return (int64_t)height * png_row_bytes(width, es);
}
TMH_DHD int64_t png_pieces(int64_t stream) { return (stream + kPngPiece - 1) / kPngPiece; }
TMH_DHD int64_t png_piece_len(int64_t stream, int64_t k) {
  return stream - k * kPngPiece < kPngPiece ? stream - k * kPngPiece : kPngPiece;
}
// A file from its pieces' bytes: signature 8, IHDR 25, 12 of length, type and
// CRC around every piece, the Adler-32's IDAT 16, IEND 12.
TMH_DHD int64_t png_file_bytes(int64_t piece_bytes, int64_t pieces) {
  return kPngHead + 12 * pieces + piece_bytes + kPngTail;
}
// No file is longer (tmh_png_bound).  From the all-stored form, which no
// piece exceeds (deflate_piece_stored_bytes): the stream's F bytes; 5 bytes
// of stored block header per segment (a stored piece has one per 65,535
// bytes: no more than its segments, kDSeg <= 65,535); per piece 5 bytes of
// sync block and 12 of chunk framing; the zlib header 2; less the 5 of the
// sync block the last piece does not have; and the 61 bytes of
// png_file_bytes: F + 5 segments + 17 pieces + 58.
TMH_DHD int64_t png_bound(int height, int width, int es) {
  const int64_t f = png_stream_bytes(height, width, es);
  return f + 5 * ((f + kDSeg - 1) / kDSeg) + 17 * png_pieces(f) + 58;
}

// ---- row filters -------------------------------------------------------

TMH_DDEV uint32_t png_cost(uint32_t v) { return v < 128u ? v : 256u - v; }

TMH_DDEV uint32_t png_paeth(int a, int b, int c) {
  const int p = a + b - c;
  const int pa = p > a ? p - a : a - p, pb = p > b ? p - b : b - p, pc = p > c ? p - c : c - p;
  return (uint32_t)(pa <= pb && pa <= pc ? a : pb <= pc ? b : c);
}

// the five filtered values of stream byte x with left a, above b, above left c
TMH_DDEV void png_filtered(uint32_t x, uint32_t a, uint32_t b, uint32_t c, uint32_t f[5]) {
  f[0] = x;
  f[1] = (x - a) & 0xFFu;
  f[2] = (x - b) & 0xFFu;
  f[3] = (x - ((a + b) >> 1)) & 0xFFu;
  f[4] = (x - png_paeth((int)a, (int)b, (int)c)) & 0xFFu;
}

// 16 bytes of a row as four words of stream bytes (16-bit samples: high byte first)
TMH_DDEV void png_load16(const uint8_t* p, int es, uint32_t v[4]) {
  typedef uint32_t PV4 __attribute__((vector_size(16)));
  const PV4 q = *reinterpret_cast<const PV4*>(p);
  for (int k = 0; k < 4; ++k)
    v[k] = es == 2 ? ((q[k] & 0x00FF00FFu) << 8) | ((q[k] >> 8) & 0x00FF00FFu) : q[k];
}
// the last stream word before byte j of a row (j a multiple of 16; zero at the row's start)
TMH_DDEV uint32_t png_left_word(const uint8_t* p, int64_t j, int es) {
  if (!p || j == 0) return 0;
  uint32_t q;
  __builtin_memcpy(&q, p + j - 4, 4);
  return es == 2 ? ((q & 0x00FF00FFu) << 8) | ((q >> 8) & 0x00FF00FFu) : q;
}
TMH_DDEV uint32_t png_byte(const uint32_t v[4], int k) { return (v[k >> 2] >> (8 * (k & 3))) & 0xFFu; }

// The five filtered values of the 16 stream bytes at j (vector form: rows
// 16-byte aligned, their bytes a multiple of 16): costs added to sum, and the
// bytes of filter `type` packed into out when it is not NULL.
TMH_DDEV void png_group16(const uint8_t* row, const uint8_t* up, int64_t j, int es, uint64_t sum[5],
                          int type, uint32_t out[4]) {
  uint32_t x[4], b[4] = {0, 0, 0, 0};
  png_load16(row + j, es, x);
  if (up) png_load16(up + j, es, b);
  const uint32_t xl = png_left_word(row, j, es), bl = png_left_word(up, j, es);
  uint32_t o[4] = {0, 0, 0, 0}, s[5] = {0, 0, 0, 0, 0};
  for (int k = 0; k < 16; ++k) {
    const uint32_t a = k >= es ? png_byte(x, k - es) : (xl >> (8 * (4 - es + k))) & 0xFFu;
    const uint32_t c = k >= es ? png_byte(b, k - es) : (bl >> (8 * (4 - es + k))) & 0xFFu;
    uint32_t f[5];
    png_filtered(png_byte(x, k), a, png_byte(b, k), c, f);
    for (int t = 0; t < 5; ++t) s[t] += png_cost(f[t]);
    const uint32_t pick = type == 0 ? f[0] : type == 1 ? f[1] : type == 2 ? f[2] : type == 3 ? f[3] : f[4];
    o[k >> 2] |= pick << (8 * (k & 3));
  }
  for (int t = 0; t < 5; ++t) sum[t] += s[t];
  if (out)
    for (int k = 0; k < 4; ++k) out[k] = o[k];
}

// stream byte j of a row (byte form)
TMH_DDEV uint32_t png_sbyte(const uint8_t* row, int64_t j, int es) { return row[es == 2 ? j ^ 1 : j]; }

TMH_DDEV void png_byte5(const uint8_t* row, const uint8_t* up, int64_t j, int es, uint32_t f[5]) {
  const uint32_t x = png_sbyte(row, j, es), a = j >= es ? png_sbyte(row, j - es, es) : 0u;
  const uint32_t b = up ? png_sbyte(up, j, es) : 0u, c = up && j >= es ? png_sbyte(up, j - es, es) : 0u;
  png_filtered(x, a, b, c, f);
}

// One row by the nl lanes of a wave: row and up (NULL for the first row) are
// the raw rows of nb = width * es bytes; out gets the type and the nb filtered
// bytes.  Two passes over the row: the five sums and the choice, then the
// chosen filter's bytes.
TMH_DDEV void png_filter_row(const uint8_t* row, const uint8_t* up, int64_t nb, int es,
                             uint8_t* out, int lane, int nl) {
  const bool v16 = (nb & 15) == 0 && (reinterpret_cast<uintptr_t>(row) & 15) == 0;
  uint64_t sum[5] = {0, 0, 0, 0, 0};
  if (v16) {
    for (int64_t j = 16 * (int64_t)lane; j < nb; j += 16 * (int64_t)nl)
      png_group16(row, up, j, es, sum, 0, nullptr);
  } else {
    for (int64_t j = lane; j < nb; j += nl) {
      uint32_t f[5];
      png_byte5(row, up, j, es, f);
      for (int t = 0; t < 5; ++t) sum[t] += png_cost(f[t]);
    }
  }
  int type = 0;
  uint64_t best = 0;
  for (int t = 0; t < 5; ++t) {
    const uint64_t s = TMH_PSUM64(sum[t]);
    if (t == 0 || s < best) best = s, type = t;
  }
  if (lane == 0) out[0] = (uint8_t)type;
  if (v16) {
    for (int64_t j = 16 * (int64_t)lane; j < nb; j += 16 * (int64_t)nl) {
      uint32_t o[4];
      png_group16(row, up, j, es, sum, type, o);
      __builtin_memcpy(out + 1 + j, o, 16);  // the stream's rows are 1 + nb bytes: not aligned
    }
  } else {
    for (int64_t j = lane; j < nb; j += nl) {
      uint32_t f[5];
      png_byte5(row, up, j, es, f);
      out[1 + j] = (uint8_t)(type == 0 ? f[0] : type == 1 ? f[1] : type == 2 ? f[2] : type == 3 ? f[3] : f[4]);
    }
  }
}

// ---- CRC-32 (IEEE, reflected: zlib.crc32) ------------------------------

constexpr uint32_t kPngPoly = 0xEDB88320u;
constexpr uint32_t kPngCrcIdat = 0x35AF061Eu;  // of the four type bytes "IDAT"

// a(x) b(x) mod P in the reflected representation (bit 31 is x^0)
TMH_DDEV uint32_t png_mulmod(uint32_t a, uint32_t b) {
  uint32_t p = 0;
  for (uint32_t m = 1u << 31; m; m >>= 1) {
    if (a & m) p ^= b;
    b = b & 1u ? (b >> 1) ^ kPngPoly : b >> 1;
  }
  return p;
}
// x^(8 n) mod P: crc(A || B) = crc(A) x^(8 |B|) + crc(B)
TMH_DDEV uint32_t png_xpow8(uint64_t n) {
  uint32_t q = 1u << 30, p = 1u << 31;  // x, 1
  for (int i = 0; i < 3; ++i) q = png_mulmod(q, q);
  for (; n; n >>= 1) {
    if (n & 1u) p = png_mulmod(q, p);
    q = png_mulmod(q, q);
  }
  return p;
}
TMH_DDEV uint32_t png_crc_join(uint32_t crc_a, uint32_t crc_b, uint64_t len_b) {
  return png_mulmod(png_xpow8(len_b), crc_a) ^ crc_b;
}

struct PShared {
  uint32_t tab[256];  // the byte-wise table
  uint32_t part[kDMaxThreads];
};

TMH_DDEV void png_crc_table(PShared& s, int tid, int nt) {
  for (int i = tid; i < 256; i += nt) {
    uint32_t c = (uint32_t)i;
    for (int k = 0; k < 8; ++k) c = c & 1u ? (c >> 1) ^ kPngPoly : c >> 1;
    s.tab[i] = c;
  }
  TMH_DSYNC();
}

// The CRC-32 of the IDAT chunk whose data are the len bytes of the slot w, by
// all nt threads (nt a power of two; every thread gets the result).  Thread t
// takes the contiguous slice that ends (nt - 1 - t) * per bytes before the
// end, so every slice to the right of another is exactly per bytes (short or
// empty slices are at the front, where their length does not enter) and the
// slices join pairwise in log2(nt) rounds: round r multiplies the left
// partner by x^(8 per 2^r).  The slot is read past this CU's vector cache
// (the bit writer's atomics were performed in L2).
TMH_DDEV uint32_t png_crc_idat(PShared& s, const uint32_t* w, int64_t len, int tid, int nt) {
  const int64_t per = (len + nt - 1) / nt;
  int64_t e1 = len - (int64_t)(nt - 1 - tid) * per, e0 = e1 - per;
  e1 = e1 > 0 ? e1 : 0;
  e0 = e0 > 0 ? e0 : 0;
  uint32_t c = 0xFFFFFFFFu, word = 0;
  for (int64_t i = e0; i < e1; ++i) {
    if (i == e0 || (i & 3) == 0) word = TMH_DLOAD32(const_cast<uint32_t*>(&w[i >> 2]));
    c = s.tab[(c ^ (word >> (8 * (i & 3)))) & 0xFFu] ^ (c >> 8);
  }
  TMH_DSYNC();  // the last call's readers of part[0] are through
  s.part[tid] = c ^ 0xFFFFFFFFu;
  uint32_t xp = png_xpow8((uint64_t)per);
  for (int st = 1; st < nt; st <<= 1) {
    TMH_DSYNC();
    if ((tid & (2 * st - 1)) == 0) s.part[tid] = png_mulmod(xp, s.part[tid]) ^ s.part[tid + st];
    xp = png_mulmod(xp, xp);
  }
  TMH_DSYNC();
  return png_crc_join(kPngCrcIdat, s.part[0], (uint64_t)len);
}

// ---- framing ----------------------------------------------------------

TMH_DDEV void png_be32(uint8_t* d, uint32_t v) {
  d[0] = (uint8_t)(v >> 24), d[1] = (uint8_t)(v >> 16), d[2] = (uint8_t)(v >> 8), d[3] = (uint8_t)v;
}
// bit by bit: the few bytes of IHDR and of the Adler-32's IDAT (one thread)
TMH_DDEV uint32_t png_crc_short(const uint8_t* p, int n) {
  uint32_t c = 0xFFFFFFFFu;
  for (int i = 0; i < n; ++i) {
    c ^= p[i];
    for (int k = 0; k < 8; ++k) c = c & 1u ? (c >> 1) ^ kPngPoly : c >> 1;
  }
  return c ^ 0xFFFFFFFFu;
}
// signature and IHDR: kPngHead bytes (one thread)
TMH_DDEV void png_write_head(uint8_t* d, int height, int width, int es) {
  const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};
  for (int i = 0; i < 8; ++i) d[i] = sig[i];
  png_be32(d + 8, 13);
  d[12] = 'I', d[13] = 'H', d[14] = 'D', d[15] = 'R';
  png_be32(d + 16, (uint32_t)width);
  png_be32(d + 20, (uint32_t)height);
  d[24] = (uint8_t)(8 * es);  // bit depth
  d[25] = 0;                  // colour type: greyscale
  d[26] = 0, d[27] = 0, d[28] = 0;  // deflate, adaptive filtering, no interlace
  png_be32(d + 29, png_crc_short(d + 12, 17));
}
// the Adler-32's IDAT and IEND: kPngTail bytes (one thread)
TMH_DDEV void png_write_tail(uint8_t* d, uint32_t adler) {
  png_be32(d, 4);
  d[4] = 'I', d[5] = 'D', d[6] = 'A', d[7] = 'T';
  png_be32(d + 8, adler);
  png_be32(d + 12, png_crc_short(d + 4, 8));
  png_be32(d + 16, 0);
  d[20] = 'I', d[21] = 'E', d[22] = 'N', d[23] = 'D';
  png_be32(d + 24, 0xAE426082u);
}
// the frame of a piece's IDAT around its len data bytes at d + 8 (one thread)
TMH_DDEV void png_write_idat_frame(uint8_t* d, int64_t len, uint32_t crc) {
  png_be32(d, (uint32_t)len);
  d[4] = 'I', d[5] = 'D', d[6] = 'A', d[7] = 'T';
  png_be32(d + 8 + len, crc);
}

// Adler-32 of a stream from its pieces in order: (a, b) start at (1, 0); a
// piece of len bytes with sums sa = sum x, sb = sum (len - i) x_i adds
// len a + sb to b, then sa to a (mod 65521: adler32_combine's arithmetic).
TMH_DDEV void png_adler_join(uint32_t& a, uint32_t& b, uint32_t sa, uint32_t sb, int64_t len) {
  b = (uint32_t)((b + (uint64_t)(len % 65521) * a + sb) % 65521u);
  a = (a + sa) % 65521u;
}

}  // namespace

}  // namespace tmh
