// Baseline JPEG of 8-bit grayscale tiles as libjpeg writes it (jpeg_set_defaults,
// JCS_GRAYSCALE, jpeg_set_quality(q, TRUE), jfdctint.c, the Annex K Huffman
// tables, no optimisation pass): the per-block arithmetic of k_jpeg_tiles
// (jpeg_kernels.hip) -- samples, forward DCT, quantisation, symbol lengths and
// bit emission -- kept free of HIP headers so the same code also builds for
// the host (tests/jpeg_host.cpp: checked byte for byte against libjpeg-turbo's
// files on the CPU).  See jpeg_kernels.hip and DESIGN.md section 13.
//
// Below the forward path, what libjpeg decodes from such a file (jdhuff.c,
// jidctint.c jpeg_idct_islow, the range limit): the inverse DCT, the round
// trip of a block, the header walk and the symbol decoder that
// k_jpeg_roundtrip and k_jpeg_decode_tiles (jpeg_decode_kernels.hip) run, and
// tests/jpeg_decode_host.cpp on the host.  DESIGN.md section 14.
#pragma once

#include <cstdint>
#include <cstring>
#include <initializer_list>

#ifndef TMH_JHD
#define TMH_JHD __host__ __device__ __forceinline__
#endif

namespace tmh {

namespace {

constexpr int kJpegHeaderBytes = 328;  // SOI .. SOS; only H, W and the DQT bytes vary
constexpr int kJpegSofDims = 94;       // offset of SOF0's height (2 bytes), then width (2 bytes)
constexpr int kJpegCoefPitch = 33;     // words per block in LDS (32 used): an odd bank stride
constexpr int kJpegMaxBlockBits = 20 + 63 * 26;  // DC 9 + 11, every AC 16 + 10

// What a call fixes for all of its tiles: the Huffman codes by symbol, the
// quantisers, and the file header with H = W = 0.
struct JpegTables {
  uint32_t ac[256];   // (code << 8) | length of symbol (run << 4 | size); 0: no such symbol
  uint32_t dc[12];    // the same by DC category
  uint32_t recip[64];  // natural order: floor(2^32 / (8 Q)) + 1
  uint16_t qv[64];     // natural order: 8 Q
  uint8_t header[kJpegHeaderBytes];
};

// ---- host: the tables of a quality ------------------------------------------

inline void jpeg_huff_codes(const uint8_t* bits, const uint8_t* vals, uint32_t* by_symbol) {
  uint32_t code = 0;
  int k = 0;
  for (int len = 1; len <= 16; ++len) {  // T.81 Annex C
    for (int i = 0; i < bits[len - 1]; ++i) by_symbol[vals[k++]] = (code++ << 8) | (uint32_t)len;
    code <<= 1;
  }
}

// jpeg_set_quality(quality, TRUE) over the Annex K.1 luminance table; the
// K.3 / K.5 luminance Huffman tables; the header as jpeg_write_header emits it
inline void jpeg_build_tables(int quality, JpegTables* t) {
  static const uint8_t base[64] = {
      16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,
      14, 13, 16, 24, 40,  57,  69,  56,  14, 17, 22, 29, 51,  87,  80,  62,
      18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,
      49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
  static const uint8_t zigzag[64] = {
      0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
      41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
      30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
  static const uint8_t dc_bits[16] = {0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0};
  static const uint8_t dc_vals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
  static const uint8_t ac_bits[16] = {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D};
  static const uint8_t ac_vals[162] = {
      0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61,
      0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xA1, 0x08, 0x23, 0x42, 0xB1, 0xC1, 0x15, 0x52,
      0xD1, 0xF0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0A, 0x16, 0x17, 0x18, 0x19, 0x1A, 0x25,
      0x26, 0x27, 0x28, 0x29, 0x2A, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45,
      0x46, 0x47, 0x48, 0x49, 0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5A, 0x63, 0x64,
      0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x83,
      0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99,
      0x9A, 0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6,
      0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3,
      0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA, 0xE1, 0xE2, 0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8,
      0xE9, 0xEA, 0xF1, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9, 0xFA};
  memset(t, 0, sizeof(*t));
  jpeg_huff_codes(dc_bits, dc_vals, t->dc);
  jpeg_huff_codes(ac_bits, ac_vals, t->ac);
  const int q = quality < 1 ? 1 : quality > 100 ? 100 : quality;
  const int s = q < 50 ? 5000 / q : 200 - 2 * q;
  uint8_t Q[64];
  for (int i = 0; i < 64; ++i) {
    int v = (base[i] * s + 50) / 100;
    v = v < 1 ? 1 : v > 255 ? 255 : v;
    Q[i] = (uint8_t)v;
    t->qv[i] = (uint16_t)(8 * v);
    t->recip[i] = (uint32_t)((uint64_t(1) << 32) / (uint64_t)(8 * v)) + 1u;
  }
  uint8_t* h = t->header;
  int n = 0;
  const auto put = [&](std::initializer_list<int> bytes) {
    for (int b : bytes) h[n++] = (uint8_t)b;
  };
  put({0xFF, 0xD8});
  put({0xFF, 0xE0, 0, 16, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0});
  put({0xFF, 0xDB, 0, 67, 0});
  for (int k = 0; k < 64; ++k) h[n++] = Q[zigzag[k]];
  put({0xFF, 0xC0, 0, 11, 8, 0, 0, 0, 0, 1, 1, 0x11, 0});
  put({0xFF, 0xC4, 0, 19 + 12, 0x00});
  for (int i = 0; i < 16; ++i) h[n++] = dc_bits[i];
  for (int i = 0; i < 12; ++i) h[n++] = dc_vals[i];
  put({0xFF, 0xC4, 0, 19 + 162, 0x10});
  for (int i = 0; i < 16; ++i) h[n++] = ac_bits[i];
  for (int i = 0; i < 162; ++i) h[n++] = ac_vals[i];
  put({0xFF, 0xDA, 0, 8, 1, 1, 0x00, 0, 63, 0});
}

// byte i of a tile's header (H, W: the tile's ragged extent)
TMH_JHD uint8_t jpeg_header_byte(const uint8_t* header, int i, int H, int W) {
  const int k = i - kJpegSofDims;
  if (k < 0 || k > 3) return header[i];
  const int v = k < 2 ? H : W;
  return (uint8_t)((k & 1) ? v & 255 : v >> 8);
}

// ---- samples ------------------------------------------------------------------

// The 64 level-shifted samples of block (by, bx) of an H x W tile stored at
// `pitch` bytes per row (pitch a multiple of 8, at least 8 (bx + 1): the eight
// bytes of a row are read whole).  Past the tile's extent the last column,
// then the last row, are replicated: what libjpeg's edge expansion does.
TMH_JHD void jpeg_load_block(const uint8_t* tile, int pitch, int H, int W, int by, int bx,
                             int (&d)[64]) {
  const int wl = W - 1 - 8 * bx;  // block column of the tile's last column
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    const int y = 8 * by + r < H ? 8 * by + r : H - 1;
    uint64_t v;
    memcpy(&v, tile + (int64_t)y * pitch + 8 * bx, 8);
    if (wl >= 7) {
#pragma unroll
      for (int c = 0; c < 8; ++c) d[8 * r + c] = (int)((v >> (8 * c)) & 255u) - 128;
    } else {
#pragma unroll
      for (int c = 0; c < 8; ++c) d[8 * r + c] = (int)((v >> (8 * (c < wl ? c : wl))) & 255u) - 128;
    }
  }
}

// ---- forward DCT (jfdctint.c) and quantisation -----------------------------------

TMH_JHD int jpeg_descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// one 1-D pass; FIRST: the row pass (results scaled up by 2^PASS1_BITS)
template <bool FIRST>
TMH_JHD void jpeg_fdct8(int& d0, int& d1, int& d2, int& d3, int& d4, int& d5, int& d6, int& d7) {
  constexpr int kConstBits = 13, kPass1Bits = 2;
  constexpr int n = FIRST ? kConstBits - kPass1Bits : kConstBits + kPass1Bits;
  const int t0 = d0 + d7, t7 = d0 - d7, t1 = d1 + d6, t6 = d1 - d6;
  const int t2 = d2 + d5, t5 = d2 - d5, t3 = d3 + d4, t4 = d3 - d4;
  const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  if (FIRST) {
    d0 = (t10 + t11) * (1 << kPass1Bits);
    d4 = (t10 - t11) * (1 << kPass1Bits);
  } else {
    d0 = jpeg_descale(t10 + t11, kPass1Bits);
    d4 = jpeg_descale(t10 - t11, kPass1Bits);
  }
  int z1 = (t12 + t13) * 4433;
  d2 = jpeg_descale(z1 + t13 * 6270, n);
  d6 = jpeg_descale(z1 - t12 * 15137, n);
  z1 = t4 + t7;
  int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
  const int z5 = (z3 + z4) * 9633;
  const int a4 = t4 * 2446, a5 = t5 * 16819, a6 = t6 * 25172, a7 = t7 * 12299;
  z1 *= -7373;
  z2 *= -20995;
  z3 = z3 * -16069 + z5;
  z4 = z4 * -3196 + z5;
  d7 = jpeg_descale(a4 + z1 + z3, n);
  d5 = jpeg_descale(a5 + z2 + z4, n);
  d3 = jpeg_descale(a6 + z2 + z3, n);
  d1 = jpeg_descale(a7 + z1 + z4, n);
}

// sign(x) ((|x| + (qv >> 1)) / qv); the division by multiplication with
// recip = floor(2^32 / qv) + 1, exact while (|x| + qv / 2) qv < 2^32 (a
// coefficient is below 2^14, qv at most 2040)
TMH_JHD int jpeg_quantise(int x, uint32_t qv, uint32_t recip) {
  const uint32_t n = (uint32_t)(x < 0 ? -x : x) + (qv >> 1);
  const int c = (int)(((uint64_t)n * recip) >> 32);
  return x < 0 ? -c : c;
}

// coefficient k (zigzag order) of a block's 32 words: two int16 to a word
TMH_JHD int jpeg_coef(const uint32_t* zw, int k) {
  return (int16_t)(zw[k >> 1] >> (16 * (k & 1)));
}

// d: 64 level-shifted samples (natural order) -> zw[32]: quantised
// coefficients in zigzag order, two to a word.  Every index is a constant
// after unrolling.
TMH_JHD void jpeg_fdct_quantise(int (&d)[64], const JpegTables& t, uint32_t* zw) {
  const uint8_t zigzag[64] = {  // natural index of the k-th coefficient in zigzag order
      0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
      41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
      30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
#pragma unroll
  for (int r = 0; r < 8; ++r)
    jpeg_fdct8<true>(d[8 * r], d[8 * r + 1], d[8 * r + 2], d[8 * r + 3], d[8 * r + 4],
                     d[8 * r + 5], d[8 * r + 6], d[8 * r + 7]);
#pragma unroll
  for (int c = 0; c < 8; ++c)
    jpeg_fdct8<false>(d[c], d[8 + c], d[16 + c], d[24 + c], d[32 + c], d[40 + c], d[48 + c],
                      d[56 + c]);
#pragma unroll
  for (int j = 0; j < 32; ++j) {
    const int a = zigzag[2 * j], b = zigzag[2 * j + 1];
    zw[j] = ((uint32_t)jpeg_quantise(d[a], t.qv[a], t.recip[a]) & 0xFFFFu) |
            ((uint32_t)jpeg_quantise(d[b], t.qv[b], t.recip[b]) << 16);
  }
}

// ---- entropy coding ---------------------------------------------------------------

// category of v and the category's low bits (a negative v sends v - 1's)
TMH_JHD int jpeg_category(int v, uint32_t* low) {
  const uint32_t a = (uint32_t)(v < 0 ? -v : v);
  const int size = a ? 32 - __builtin_clz(a) : 0;
  *low = (uint32_t)(v < 0 ? v - 1 : v) & ((1u << size) - 1u);
  return size;
}

// The symbols of one block (zw: jpeg_fdct_quantise's words; prev_dc: the DC
// of the block before it in the tile, 0 for the first) into sink.put(bits, n),
// n <= 26: Huffman code and value bits of a symbol in one piece.  Eight
// coefficients at a time: their words are loaded together, eight zeros are
// passed over at once, and otherwise the eight zero runs, categories and code
// table entries are worked out before anything is emitted -- the table reads
// depend on the coefficients alone, so they are in flight together instead
// of one LDS round trip per symbol.
template <class Sink>
TMH_JHD void jpeg_encode_block(const uint32_t* zw, int prev_dc, const JpegTables& t, Sink& sink) {
  uint32_t dc_low;
  const int dc_size = jpeg_category(jpeg_coef(zw, 0) - prev_dc, &dc_low);
  const uint32_t dc = t.dc[dc_size];
  sink.put(((dc >> 8) << dc_size) | dc_low, (int)(dc & 255u) + dc_size);
  const uint32_t zrl = t.ac[0xF0];
  int run = 0;  // zeros since the last symbol
  for (int g = 0; g < 8; ++g) {
    uint32_t w[4] = {zw[4 * g], zw[4 * g + 1], zw[4 * g + 2], zw[4 * g + 3]};
    if (g == 0) w[0] &= 0xFFFF0000u;  // the DC is no AC coefficient ...
    if ((w[0] | w[1] | w[2] | w[3]) == 0) {
      run += g ? 8 : 7;
      continue;
    }
    int v[8], before[8], size[8];
    uint32_t low[8], e[8];
    int r = g ? run : -1;  // ... and no zero of a run
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      v[j] = (int16_t)(w[j >> 1] >> (16 * (j & 1)));
      before[j] = r;
      size[j] = jpeg_category(v[j], &low[j]);
      e[j] = t.ac[((r & 15) << 4) | size[j]];
      r = v[j] ? 0 : r + 1;
    }
    run = r;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if (v[j] == 0) continue;
      for (int z = before[j] >> 4; z > 0; --z) sink.put(zrl >> 8, (int)(zrl & 255u));
      sink.put(((e[j] >> 8) << size[j]) | low[j], (int)(e[j] & 255u) + size[j]);
    }
  }
  if (run) sink.put(t.ac[0] >> 8, (int)(t.ac[0] & 255u));  // EOB
}

struct JpegCountSink {
  int bits = 0;
  TMH_JHD void put(uint32_t, int n) { bits += n; }
};

// Bits, MSB first, into 32-bit words starting at bit `at` of `words` (zeroed;
// several blocks share their first and last word, so words are merged with
// Or::apply -- an LDS atomic on the device).  Up to 31 + 26 bits wait in acc.
template <class Or>
struct JpegBitSink {
  uint32_t* w;
  uint64_t acc = 0;
  int n;
  TMH_JHD JpegBitSink(uint32_t* words, int at) : w(words + (at >> 5)), n(at & 31) {}
  TMH_JHD void put(uint32_t bits, int len) {
    acc = (acc << len) | bits;
    n += len;
    if (n >= 32) {
      n -= 32;
      Or::apply(w++, (uint32_t)(acc >> n));
      acc &= (uint64_t(1) << n) - 1u;
    }
  }
  TMH_JHD void finish() {
    if (n) Or::apply(w, (uint32_t)(acc << (32 - n)));
  }
};

// byte i of the bit stream held in words
TMH_JHD uint32_t jpeg_stream_byte(const uint32_t* words, int i) {
  return (words[i >> 2] >> (24 - 8 * (i & 3))) & 255u;
}

// ---- decoding (jdhuff.c, jidctint.c): DESIGN.md section 14 -----------------------------

// Inverse DCT of one block as jpeg_idct_islow does it, range limit included.
// c: 64 dequantised coefficients, natural order; becomes the 64 samples 0..255.
// libjpeg works in 32-bit integers that cannot overflow for the coefficients
// an encoder of 8-bit samples produces; a corrupt file's can, so the sums and
// products here are unsigned (they wrap, bit for bit the same while nothing
// overflows) and only the descaling shift is signed.
template <bool FIRST>
TMH_JHD void jpeg_idct8(int& d0, int& d1, int& d2, int& d3, int& d4, int& d5, int& d6, int& d7) {
  constexpr int kConstBits = 13, kPass1Bits = 2;
  constexpr int n = FIRST ? kConstBits - kPass1Bits : kConstBits + kPass1Bits + 3;
  typedef uint32_t u;
  const u c0 = (u)d0, c1 = (u)d1, c2 = (u)d2, c3 = (u)d3, c4 = (u)d4, c5 = (u)d5, c6 = (u)d6,
          c7 = (u)d7;
  u z1 = (c2 + c6) * (u)4433;
  const u e2 = z1 + c6 * (u)-15137, e3 = z1 + c2 * (u)6270;
  const u e0 = (c0 + c4) << kConstBits, e1 = (c0 - c4) << kConstBits;
  const u t10 = e0 + e3, t13 = e0 - e3, t11 = e1 + e2, t12 = e1 - e2;
  z1 = c7 + c1;
  u z2 = c5 + c3, z3 = c7 + c3, z4 = c5 + c1;
  const u z5 = (z3 + z4) * (u)9633;
  u o0 = c7 * (u)2446, o1 = c5 * (u)16819, o2 = c3 * (u)25172,
    o3 = c1 * (u)12299;
  z1 = z1 * (u)-7373;
  z2 = z2 * (u)-20995;
  z3 = z3 * (u)-16069 + z5;
  z4 = z4 * (u)-3196 + z5;
  o0 += z1 + z3;
  o1 += z2 + z4;
  o2 += z2 + z3;
  o3 += z1 + z4;
  constexpr u half = 1u << (n - 1);
  d0 = (int)(t10 + o3 + half) >> n;
  d7 = (int)(t10 - o3 + half) >> n;
  d1 = (int)(t11 + o2 + half) >> n;
  d6 = (int)(t11 - o2 + half) >> n;
  d2 = (int)(t12 + o1 + half) >> n;
  d5 = (int)(t12 - o1 + half) >> n;
  d3 = (int)(t13 + o0 + half) >> n;
  d4 = (int)(t13 - o0 + half) >> n;
}

TMH_JHD void jpeg_idct_block(int (&c)[64]) {
#pragma unroll
  for (int x = 0; x < 8; ++x)  // pass 1: columns
    jpeg_idct8<true>(c[x], c[8 + x], c[16 + x], c[24 + x], c[32 + x], c[40 + x], c[48 + x],
                     c[56 + x]);
#pragma unroll
  for (int r = 0; r < 8; ++r)  // pass 2: rows
    jpeg_idct8<false>(c[8 * r], c[8 * r + 1], c[8 * r + 2], c[8 * r + 3], c[8 * r + 4],
                      c[8 * r + 5], c[8 * r + 6], c[8 * r + 7]);
#pragma unroll
  for (int i = 0; i < 64; ++i) {
    const int v = c[i] + 128;
    c[i] = v < 0 ? 0 : v > 255 ? 255 : v;
  }
}

// d: 64 level-shifted samples -> the 64 samples libjpeg decodes from the file
// the encoder writes for them (Huffman coding is lossless: the forward DCT,
// the quantiser, the quantiser's inverse and the inverse DCT).  t: anything
// with JpegTables' qv and recip.
template <class Tables>
TMH_JHD void jpeg_roundtrip_block(int (&d)[64], const Tables& t) {
#pragma unroll
  for (int r = 0; r < 8; ++r)
    jpeg_fdct8<true>(d[8 * r], d[8 * r + 1], d[8 * r + 2], d[8 * r + 3], d[8 * r + 4],
                     d[8 * r + 5], d[8 * r + 6], d[8 * r + 7]);
#pragma unroll
  for (int c = 0; c < 8; ++c)
    jpeg_fdct8<false>(d[c], d[8 + c], d[16 + c], d[24 + c], d[32 + c], d[40 + c], d[48 + c],
                      d[56 + c]);
#pragma unroll
  for (int i = 0; i < 64; ++i) d[i] = jpeg_quantise(d[i], t.qv[i], t.recip[i]) * (int)(t.qv[i] >> 3);
  jpeg_idct_block(d);
}

// row r of a decoded block (samples 0..255) as eight bytes; bytes at and after
// column `keep` (the tile's extent within the block) are 0
TMH_JHD uint64_t jpeg_pack_row(const int (&d)[64], int r, int keep) {
  uint64_t v = 0;
#pragma unroll
  for (int c = 0; c < 8; ++c) v |= (uint64_t)(c < keep ? d[8 * r + c] : 0) << (8 * c);
  return v;
}

// Status of a file: 0 decoded, 1 well formed but outside what is decoded, 2 corrupt.
constexpr int kJpegOk = 0, kJpegUnsupported = 1, kJpegCorrupt = 2;

// What the decoder fixes for every file: the Annex K luminance tables as
// lookups.  A code of up to 9 bits is found by the next 9 bits of the stream:
// (symbol << 8) | length, 0 when the code is longer (AC only); those by the
// classic maxcode / valptr walk over lengths 10..16.
struct JpegDecodeTables {
  uint16_t dc[512];
  uint16_t ac[512];
  int32_t ac_maxcode[17];  // largest code of a length, -1: none
  int32_t ac_valoff[17];   // index of a length's first symbol minus its first code
  uint8_t ac_vals[162];
  uint8_t dc_bits[16], dc_vals[12], ac_bits[16];  // as a DHT segment carries them
  uint8_t zigzag[64];
};

inline void jpeg_build_decode_tables(JpegDecodeTables* t) {
  JpegTables e;
  jpeg_build_tables(95, &e);
  memset(t, 0, sizeof(*t));
  // the encoder's header holds the two DHT segments: at 102 and 135, five bytes before the counts
  const uint8_t* h = e.header;
  memcpy(t->dc_bits, h + 107, 16);
  memcpy(t->dc_vals, h + 123, 12);
  memcpy(t->ac_bits, h + 140, 16);
  memcpy(t->ac_vals, h + 156, 162);
  static const uint8_t zigzag[64] = {
      0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
      41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
      30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
  memcpy(t->zigzag, zigzag, 64);
  for (int pass = 0; pass < 2; ++pass) {
    const uint8_t* bits = pass ? t->ac_bits : t->dc_bits;
    const uint8_t* vals = pass ? t->ac_vals : t->dc_vals;
    uint16_t* lut = pass ? t->ac : t->dc;
    uint32_t code = 0;
    int k = 0;
    for (int len = 1; len <= 16; ++len) {
      if (pass) {
        t->ac_valoff[len] = k - (int)code;
        t->ac_maxcode[len] = bits[len - 1] ? (int)code + bits[len - 1] - 1 : -1;
      }
      for (int i = 0; i < bits[len - 1]; ++i, ++k, ++code)
        if (len <= 9)
          for (uint32_t f = 0; f < (1u << (9 - len)); ++f)
            lut[(code << (9 - len)) | f] = (uint16_t)((vals[k] << 8) | len);
      code <<= 1;
    }
  }
}

struct JpegFileInfo {
  int height, width;
  int64_t scan;     // offset of the first entropy-coded byte
  uint8_t q[64];    // the quantisers, natural order
};

// The markers of file f[0 .. n) up to and including SOS.  Corruption (a
// segment that does not fit, a malformed one) ends the walk with status 2 at
// once; anything well formed but outside the decoded set is remembered and
// reported as status 1 when SOS is reached.  No byte outside [0, n) is read.
TMH_JHD int jpeg_parse_header(const uint8_t* f, int64_t n, const JpegDecodeTables& t,
                              JpegFileInfo* info) {
  info->height = info->width = 0;
  info->scan = 0;
  if (n < 4 || f[0] != 0xFF || f[1] != 0xD8) return kJpegCorrupt;
  bool unsupported = false, have_q = false, have_sof = false, have_dc = false, have_ac = false;
  int component = 0;
  int64_t at = 2;
  for (;;) {
    if (at + 4 > n || f[at] != 0xFF) return kJpegCorrupt;
    const int m = f[at + 1];
    const int64_t len = ((int64_t)f[at + 2] << 8) | f[at + 3];
    const int64_t seg = at + 4, end = at + 2 + len;  // the segment's payload
    if (m == 0xFF || m == 0x00 || m == 0x01 || (m >= 0xD0 && m <= 0xD9)) return kJpegCorrupt;
    if (len < 2 || end > n) return kJpegCorrupt;
    if (m == 0xDB) {
      int64_t p = seg;
      while (p < end) {
        const int pq = f[p] >> 4, tq = f[p] & 15;
        if (pq > 1 || tq > 3) return kJpegCorrupt;
        const int64_t bytes = pq ? 128 : 64;
        if (p + 1 + bytes > end) return kJpegCorrupt;
        if (tq == 0) {
          if (pq) {
            unsupported = true;
          } else {
            for (int k = 0; k < 64; ++k) {
              if (f[p + 1 + k] == 0) return kJpegCorrupt;
              info->q[t.zigzag[k]] = f[p + 1 + k];
            }
            have_q = true;
          }
        }
        p += 1 + bytes;
      }
    } else if (m == 0xC0) {
      if (have_sof || len < 8) return kJpegCorrupt;
      const int nf = f[seg + 5];
      if (len != 8 + 3 * nf || nf == 0) return kJpegCorrupt;
      have_sof = true;
      info->height = (f[seg + 1] << 8) | f[seg + 2];
      info->width = (f[seg + 3] << 8) | f[seg + 4];
      component = f[seg + 6];
      if (f[seg] != 8 || nf != 1 || f[seg + 7] != 0x11 || f[seg + 8] != 0 || info->height < 1 ||
          info->height > 256 || info->width < 1 || info->width > 256)
        unsupported = true;
    } else if ((m >= 0xC1 && m <= 0xCF && m != 0xC4) || m == 0xDC) {
      if (m != 0xCC && m != 0xDC) have_sof = true;
      unsupported = true;  // other frame types, arithmetic conditioning, DNL
    } else if (m == 0xC4) {
      int64_t p = seg;
      while (p < end) {
        const int tc = f[p] >> 4, th = f[p] & 15;
        if (tc > 1 || th > 3 || p + 17 > end) return kJpegCorrupt;
        int count = 0;
        for (int i = 0; i < 16; ++i) count += f[p + 1 + i];
        if (count > 256 || p + 17 + count > end) return kJpegCorrupt;
        if (th == 0) {
          const uint8_t* bits = tc ? t.ac_bits : t.dc_bits;
          const uint8_t* vals = tc ? t.ac_vals : t.dc_vals;
          bool same = count == (tc ? 162 : 12);
          for (int i = 0; i < 16; ++i) same = same && f[p + 1 + i] == bits[i];
          for (int i = 0; same && i < count; ++i) same = f[p + 17 + i] == vals[i];
          if (!same) unsupported = true;
          (tc ? have_ac : have_dc) = true;
        }
        p += 17 + count;
      }
    } else if (m == 0xDD) {
      if (len != 4) return kJpegCorrupt;
      if (f[seg] | f[seg + 1]) unsupported = true;
    } else if (m == 0xDA) {
      if (!have_sof || len < 6) return kJpegCorrupt;
      if (unsupported) return kJpegUnsupported;
      const int ns = f[seg];
      if (len != 6 + 2 * ns) return kJpegCorrupt;
      if (ns != 1) return kJpegUnsupported;
      if (f[seg + 1] != component) return kJpegCorrupt;
      if (f[seg + 2] != 0 || f[seg + 3] != 0 || f[seg + 4] != 63 || f[seg + 5] != 0)
        return kJpegUnsupported;
      if (!have_q || !have_dc || !have_ac) return kJpegUnsupported;
      info->scan = end;
      return kJpegOk;
    }
    // APPn, COM and every other segment: passed over
    at = end;
  }
}

// The entropy-coded bytes f[pos .. end) as bits, most significant first.
// 0xFF 0x00 is one 0xFF byte; any other 0xFF xx is a marker, where -- as at
// `end` -- the bits stop.  `n` counts real bits only: asking for more fails.
struct JpegBitReader {
  const uint8_t* f;
  int64_t pos, end;
  uint32_t acc = 0;  // the next bits at the top, zeros below the n-th
  int n = 0;
  bool stop = false;
  TMH_JHD JpegBitReader(const uint8_t* file, int64_t at, int64_t size)
      : f(file), pos(at), end(size) {}
  TMH_JHD void fill() {
    while (n <= 24 && !stop) {
      if (pos >= end) {
        stop = true;
        break;
      }
      const uint32_t b = f[pos];
      if (b == 0xFF) {
        if (pos + 1 >= end || f[pos + 1] != 0) {
          stop = true;
          break;
        }
        pos += 2;
      } else {
        pos += 1;
      }
      acc |= b << (24 - n);
      n += 8;
    }
  }
  TMH_JHD uint32_t peek(int k) const { return acc >> (32 - k); }  // 1 <= k <= 16, after fill()
  TMH_JHD bool skip(int k) {
    if (k > n) return false;
    acc <<= k;
    n -= k;
    return true;
  }
  // after the last block: only the padding of the last byte is left, then EOI
  TMH_JHD bool at_eoi() {
    fill();
    return n < 8 && stop && pos + 1 < end && f[pos] == 0xFF && f[pos + 1] == 0xD9;
  }
};

// the `size` bits after a symbol as the value they stand for (T.81 F.2.2.1 EXTEND)
TMH_JHD bool jpeg_receive(JpegBitReader& r, int size, int* v) {
  *v = 0;
  if (size == 0) return true;
  r.fill();
  const int x = (int)r.peek(size);
  if (!r.skip(size)) return false;
  *v = x < (1 << (size - 1)) ? x - (1 << size) + 1 : x;
  return true;
}

// One block's symbols -> coefficient k (zigzag order) into put(natural index,
// value); nothing is put for a zero.  *dc: the predictor, updated.  Returns
// kJpegOk or kJpegCorrupt: the bits end early, a pattern is no code, a DC
// category above 11 or an AC size above 10, a DC outside -2048..2047 (none of
// an 8-bit picture's is), a coefficient index past 63 -- checked before put().
template <class Put>
TMH_JHD int jpeg_decode_block(JpegBitReader& r, const JpegDecodeTables& t, int* dc, Put& put) {
  r.fill();
  uint32_t e = t.dc[r.peek(9)];
  if (e == 0 || !r.skip((int)(e & 255u))) return kJpegCorrupt;
  int s = (int)(e >> 8), v;
  if (s > 11 || !jpeg_receive(r, s, &v)) return kJpegCorrupt;
  *dc += v;
  if (*dc < -2048 || *dc > 2047) return kJpegCorrupt;
  if (*dc) put(0, *dc);
  int k = 1;
  while (k < 64) {
    r.fill();
    e = t.ac[r.peek(9)];
    int sym, len;
    if (e) {
      sym = (int)(e >> 8);
      len = (int)(e & 255u);
    } else {
      const int code16 = (int)r.peek(16);
      for (len = 10; len <= 16; ++len)
        if ((code16 >> (16 - len)) <= t.ac_maxcode[len]) break;
      if (len > 16) return kJpegCorrupt;
      sym = t.ac_vals[(code16 >> (16 - len)) + t.ac_valoff[len]];
    }
    if (!r.skip(len)) return kJpegCorrupt;
    const int run = sym >> 4;
    s = sym & 15;
    if (s == 0) {
      if (run != 15) break;  // EOB (the tables hold no other symbol of size 0)
      k += 16;
      if (k > 64) return kJpegCorrupt;
      continue;
    }
    k += run;
    if (s > 10 || k > 63 || !jpeg_receive(r, s, &v)) return kJpegCorrupt;
    put((int)t.zigzag[k], v);
    ++k;
  }
  return kJpegOk;
}

}  // namespace

}  // namespace tmh
