// Deflate encode of one zlib stream per workgroup: the core of
// k_deflate_chunks (deflate_kernels.hip), kept free of HIP headers so the
// same code also builds for the host (tests/deflate_host.cpp: the encoder
// checked against zlib's inflate on CPU).  The mirror of inflate_core.h.
//
// Every function here is called by all nt threads of a workgroup (host:
// nt = 1, the barriers are empty).  No result depends on nt or on the order
// in which lanes arrive, so the host build and the kernel emit the same bytes
// (DESIGN §18 has the rules):
//  - a chunk is cut into segments of kDSeg bytes (staged in LDS); a segment
//    is one block of the stream, matches do not cross segments;
//  - match finder: a 4-byte hash, one bucket entry = the most recent position
//    of an EARLIER batch of kDBatch positions (every position of a batch
//    looks up, then every position inserts with max), plus the fixed
//    distances 1, 2 and 4 (runs, constant uint16, constant 4-byte groups,
//    which a batch cannot find in itself).  Longest wins, ties to the nearer.
//    Minimum match 4, maximum 258, greedy parse from the segment's start;
//  - per block the smallest of: dynamic Huffman over the parse, dynamic
//    Huffman over literals only, stored -- from exact bit counts;
//  - a stream longer than the all-stored stream is rewritten as stored
//    blocks of 65,535 bytes, so deflate_bound() always holds.
#pragma once

#include <cstdint>

#include "../../include/tmhip.h"

#ifndef TMH_DDEV
#define TMH_DDEV __device__
#define TMH_DHD __host__ __device__ __forceinline__
#define TMH_DSYNC() __syncthreads()
// global writes of this workgroup visible to its other threads
#define TMH_DSYNC_GLOBAL() \
  do {                     \
    __threadfence();       \
    __syncthreads();       \
  } while (0)
#define TMH_DOR32(p, v) atomicOr((p), (v))
#define TMH_DMAX32(p, v) atomicMax((p), (v))
#define TMH_DADD32(p, v) atomicAdd((p), (v))
// a load that sees the other lanes' atomics (not this CU's cached line)
#define TMH_DLOAD32(p) __hip_atomic_load((p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#endif

namespace tmh {

namespace {

constexpr int kDSeg = 49152;   // bytes of a segment (<= 65,535: a stored segment is one block)
constexpr int kDBatch = 256;   // positions that look up before any of them inserts
constexpr int kDHashBits = 15;  // buckets in global scratch (LDS holds the bytes and lengths)
constexpr int kDMinMatch = 4, kDMaxMatch = 258;
constexpr int kDMaxThreads = 256;
constexpr int kDLl = 286, kDDist = 30, kDCl = 19;
constexpr int kDModeMatch = 0, kDModeLit = 1, kDModeStored = 2;

// the slot of a chunk's stream: never more than this many bytes (tmh_deflate_bound)
TMH_DHD int64_t deflate_bound(int64_t raw_len) {
  const int64_t n = raw_len > 1 ? raw_len : 1;
  return raw_len + 5 * ((n + 65534) / 65535) + 6;
}
// Slot stride in bytes.  Before the stored rewrite a stream of many segments
// may pass the bound: a segment's block is never worse than stored, at most 6
// bytes over its own (3 header bits, the padding, LEN, NLEN).  32-bit words,
// one spare word for the bit writer's carry.
TMH_DHD int64_t deflate_slot_bytes(int64_t raw_max) {
  const int64_t nseg = raw_max > 0 ? (raw_max + kDSeg - 1) / kDSeg : 1;
  const int64_t worst = raw_max + 6 * nseg + 6, bound = deflate_bound(raw_max);
  return (((worst > bound ? worst : bound) + 3) & ~int64_t(3)) + 8;
}

struct DShared {
  alignas(16) uint8_t raw[kDSeg + 16];  // the segment (zero padded: hashes read 3 bytes past)
  uint8_t lenb[kDSeg];                  // per position: match length - 3, 0 = no match
  uint32_t tok[kDSeg / 32];             // bit p: a token of the greedy parse starts at p
  uint32_t hist_ll[2][288];             // [kDModeMatch | kDModeLit]
  uint32_t hist_d[32];
  uint32_t hist_cl[2][kDCl];
  uint8_t ll_len[2][288];
  uint16_t ll_code[2][288];
  uint8_t d_len[32];
  uint16_t d_code[32];
  uint8_t cl_len[2][kDCl];
  uint16_t cl_code[2][kDCl];
  uint8_t seq_sym[2][320];  // the run-length coded code lengths of a block header
  uint8_t seq_ext[2][320];
  int seq_n[2], hlit[2], hdist[2];
  uint16_t order[288];  // code construction: used symbols by ascending (count, symbol)
  uint32_t work[288];
  int cnt[64];          // code construction: codes per length
  uint32_t part[kDMaxThreads + 1];
  uint64_t red[2][kDMaxThreads];
  int mode;
  uint64_t bitpos;  // stream bits written so far
};

TMH_DDEV uint32_t dhash4(const uint8_t* p) {
  const uint32_t v = (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
  return (v * 2654435761u) >> (32 - kDHashBits);
}

TMH_DDEV uint32_t dbitrev(uint32_t code, int len) {
  uint32_t r = 0;
  for (int i = 0; i < len; ++i) r |= ((code >> i) & 1u) << (len - 1 - i);
  return r;
}

// RFC 1951 3.2.5: the length symbol of a match length, its extra bits
TMH_DDEV void dlen_sym(int len, int& sym, int& nx, uint32_t& x) {
  const uint32_t l = (uint32_t)(len - 3);
  if (l < 8) {
    sym = 257 + (int)l, nx = 0, x = 0;
  } else if (len == 258) {
    sym = 285, nx = 0, x = 0;
  } else {
    const int nb = 31 - __builtin_clz(l);
    sym = 257 + 4 * (nb - 1) + (int)((l >> (nb - 2)) & 3u);
    nx = nb - 2;
    x = l & ((1u << nx) - 1u);
  }
}
TMH_DDEV void ddist_sym(int dist, int& sym, int& nx, uint32_t& x) {
  const uint32_t d = (uint32_t)(dist - 1);
  if (d < 4) {
    sym = (int)d, nx = 0, x = 0;
  } else {
    const int nb = 31 - __builtin_clz(d);
    sym = 2 * nb + (int)((d >> (nb - 1)) & 1u);
    nx = nb - 1;
    x = d & ((1u << nx) - 1u);
  }
}
TMH_DDEV int dll_extra(int sym) { return sym < 265 || sym == 285 ? 0 : (sym - 261) >> 2; }
TMH_DDEV int ddist_extra(int sym) { return sym < 4 ? 0 : (sym >> 1) - 1; }

// n <= 32 bits of v at stream bit `pos` of the zeroed slot (any thread, any position)
TMH_DDEV void dput(uint32_t* w, uint64_t pos, uint32_t v, int n) {
  if (n == 0) return;
  const uint64_t x = (uint64_t)v << (pos & 31u);
  TMH_DOR32(&w[pos >> 5], (uint32_t)x);
  if (x >> 32) TMH_DOR32(&w[(pos >> 5) + 1], (uint32_t)(x >> 32));
}

// A thread's run of consecutive bits: words it covers whole are plain stores,
// the first and the last (shared with the neighbours' runs) are OR-ed in.
struct DBitW {
  uint32_t* w;
  uint64_t acc;
  int nacc;       // bits in acc; bit 0 of acc is stream bit 32 * word + lead
  uint64_t word;
  bool whole;     // the next flushed word starts at this run's own bit 0 of it
};
TMH_DDEV void dbw_open(DBitW& b, uint32_t* w, uint64_t pos) {
  b.w = w;
  b.word = pos >> 5;
  b.nacc = (int)(pos & 31u);
  b.acc = 0;
  b.whole = b.nacc == 0;
}
TMH_DDEV void dbw_put(DBitW& b, uint32_t v, int n) {  // n <= 32
  b.acc |= (uint64_t)v << b.nacc;
  b.nacc += n;
  if (b.nacc >= 32) {
    if (b.whole) b.w[b.word] = (uint32_t)b.acc;
    else TMH_DOR32(&b.w[b.word], (uint32_t)b.acc);
    b.whole = true;
    b.word += 1;
    b.acc >>= 32;
    b.nacc -= 32;
  }
}
TMH_DDEV void dbw_close(DBitW& b) {
  if (b.nacc > 0 && (uint32_t)b.acc) TMH_DOR32(&b.w[b.word], (uint32_t)b.acc);
}

// Length-limited Huffman code lengths of hist[0..n) into out[0..n): the
// in-place minimum-redundancy construction of Moffat and Katajainen over the
// used symbols sorted by (count, symbol), then lengths past maxbits moved
// down and the Kraft sum repaired from the longest codes (as miniz does).  A
// code of one used symbol gets a second, unused, one-bit code (a complete
// code: what zlib's inflate asks of the literal and the code-length codes).
TMH_DDEV void dbuild_code(DShared& z, const uint32_t* hist, int n, int maxbits, uint8_t* out,
                          int tid, int nt) {
  TMH_DSYNC();
  for (int s = tid; s < n; s += nt) {
    const uint32_t c = hist[s];
    out[s] = 0;
    if (c) {
      int rank = 0;
      for (int t = 0; t < n; ++t) {
        const uint32_t ct = hist[t];
        rank += (ct && (ct < c || (ct == c && t < s))) ? 1 : 0;
      }
      z.order[rank] = (uint16_t)s;
    }
  }
  TMH_DSYNC();
  if (tid == 0) {
    int m = 0;
    for (int s = 0; s < n; ++s) m += hist[s] ? 1 : 0;
    if (m == 0) {
      out[0] = 1;
    } else if (m == 1) {
      out[z.order[0]] = 1;
      out[z.order[0] == 0 ? 1 : 0] = 1;
    } else {
      uint32_t* A = z.work;
      for (int i = 0; i < m; ++i) A[i] = hist[z.order[i]];
      A[0] += A[1];
      int root = 0, leaf = 2, next;
      for (next = 1; next < m - 1; ++next) {
        if (leaf >= m || A[root] < A[leaf]) {
          A[next] = A[root];
          A[root++] = (uint32_t)next;
        } else {
          A[next] = A[leaf++];
        }
        if (leaf >= m || (root < next && A[root] < A[leaf])) {
          A[next] += A[root];
          A[root++] = (uint32_t)next;
        } else {
          A[next] += A[leaf++];
        }
      }
      A[m - 2] = 0;
      for (next = m - 3; next >= 0; --next) A[next] = A[A[next]] + 1;
      int avbl = 1, used = 0, dpth = 0;
      root = m - 2;
      next = m - 1;
      while (avbl > 0) {
        while (root >= 0 && (int)A[root] == dpth) {
          ++used;
          --root;
        }
        while (avbl > used) {
          A[next--] = (uint32_t)dpth;
          --avbl;
        }
        avbl = 2 * used;
        ++dpth;
        used = 0;
      }
      // A[i]: the length of the i-th rarest symbol (non-increasing in i)
      int* cnt = z.cnt;  // (LDS: a private array indexed by a variable lives in scratch memory)
      for (int l = 0; l < 64; ++l) cnt[l] = 0;
      for (int i = 0; i < m; ++i) cnt[A[i] < 63u ? A[i] : 63u] += 1;
      for (int l = maxbits + 1; l < 64; ++l) cnt[maxbits] += cnt[l];
      uint32_t total = 0;
      for (int l = maxbits; l > 0; --l) total += (uint32_t)cnt[l] << (maxbits - l);
      while (total != (1u << maxbits)) {
        cnt[maxbits] -= 1;
        for (int l = maxbits - 1; l > 0; --l)
          if (cnt[l]) {
            cnt[l] -= 1;
            cnt[l + 1] += 2;
            break;
          }
        total -= 1;
      }
      int i = 0;
      for (int l = maxbits; l > 0; --l)
        for (int c = 0; c < cnt[l]; ++c) out[z.order[i++]] = (uint8_t)l;
    }
  }
  TMH_DSYNC();
}

// canonical codes of the lengths, in stream bit order (thread 0)
TMH_DDEV void dassign_codes(const uint8_t* len, int n, uint16_t* code) {
  uint32_t cnt[16], nextc[16];
  for (int l = 0; l < 16; ++l) cnt[l] = 0;
  for (int s = 0; s < n; ++s) cnt[len[s]] += 1;
  cnt[0] = 0;
  uint32_t c = 0;
  nextc[0] = 0;
  for (int l = 1; l < 16; ++l) {
    c = (c + cnt[l - 1]) << 1;
    nextc[l] = c;
  }
  for (int s = 0; s < n; ++s) {
    const int l = len[s];
    code[s] = l ? (uint16_t)dbitrev(nextc[l]++, l) : (uint16_t)0;
  }
}

// the code lengths of a dynamic block's two codes, run-length coded with the
// symbols 16 / 17 / 18 (thread 0); counts the code-length symbols
TMH_DDEV void drle_header(DShared& z, int v) {
  int hlit = kDLl, hdist = kDDist;
  while (hlit > 257 && z.ll_len[v][hlit - 1] == 0) --hlit;
  while (hdist > 1 && z.d_len[hdist - 1] == 0) --hdist;
  if (v == kDModeLit) hdist = 1;  // no matches: one distance code, of length 1
  z.hlit[v] = hlit;
  z.hdist[v] = hdist;
  const int total = hlit + hdist;
  int k = 0;
  for (int s = 0; s < kDCl; ++s) z.hist_cl[v][s] = 0;
  int i = 0;
  while (i < total) {
    const int val = i < hlit ? z.ll_len[v][i] : (v == kDModeLit ? 1 : z.d_len[i - hlit]);
    int run = 1;
    while (i + run < total) {
      const int j = i + run;
      const int vj = j < hlit ? z.ll_len[v][j] : (v == kDModeLit ? 1 : z.d_len[j - hlit]);
      if (vj != val) break;
      ++run;
    }
    i += run;
    if (val == 0) {
      while (run >= 11) {
        const int r = run < 138 ? run : 138;
        z.seq_sym[v][k] = 18, z.seq_ext[v][k++] = (uint8_t)(r - 11);
        z.hist_cl[v][18] += 1;
        run -= r;
      }
      if (run >= 3) {
        z.seq_sym[v][k] = 17, z.seq_ext[v][k++] = (uint8_t)(run - 3);
        z.hist_cl[v][17] += 1;
        run = 0;
      }
    } else {
      z.seq_sym[v][k] = (uint8_t)val, z.seq_ext[v][k++] = 0;
      z.hist_cl[v][val] += 1;
      run -= 1;
      while (run >= 3) {
        const int r = run < 6 ? run : 6;
        z.seq_sym[v][k] = 16, z.seq_ext[v][k++] = (uint8_t)(r - 3);
        z.hist_cl[v][16] += 1;
        run -= r;
      }
    }
    for (; run > 0; --run) {
      z.seq_sym[v][k] = (uint8_t)val, z.seq_ext[v][k++] = 0;
      z.hist_cl[v][val] += 1;
    }
  }
  z.seq_n[v] = k;
}

constexpr uint8_t kDClOrder[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

TMH_DDEV int dhclen(const DShared& z, int v) {
  int h = kDCl;
  while (h > 4 && z.cl_len[v][kDClOrder[h - 1]] == 0) --h;
  return h;
}

// exact bits of the dynamic block of variant v, its 3-bit block header included (thread 0)
TMH_DDEV uint64_t ddyn_bits(const DShared& z, int v) {
  uint64_t bits = 3 + 14 + 3 * (uint64_t)dhclen(z, v);
  for (int s = 0; s < kDCl; ++s)
    bits += (uint64_t)z.hist_cl[v][s] * (z.cl_len[v][s] + (s == 16 ? 2 : s == 17 ? 3 : s == 18 ? 7 : 0));
  for (int s = 0; s < kDLl; ++s)
    bits += (uint64_t)z.hist_ll[v][s] * (z.ll_len[v][s] + (s > 256 ? dll_extra(s) : 0));
  if (v == kDModeMatch)
    for (int s = 0; s < kDDist; ++s) bits += (uint64_t)z.hist_d[s] * (z.d_len[s] + ddist_extra(s));
  return bits;
}

// the dynamic block's header at pos (thread 0); returns the position after it
TMH_DDEV uint64_t demit_dyn_header(const DShared& z, int v, uint32_t* w, uint64_t pos, int last) {
  dput(w, pos, (uint32_t)last | 2u << 1, 3), pos += 3;
  const int hclen = dhclen(z, v);
  dput(w, pos, (uint32_t)(z.hlit[v] - 257), 5), pos += 5;
  dput(w, pos, (uint32_t)(z.hdist[v] - 1), 5), pos += 5;
  dput(w, pos, (uint32_t)(hclen - 4), 4), pos += 4;
  for (int i = 0; i < hclen; ++i) dput(w, pos, z.cl_len[v][kDClOrder[i]], 3), pos += 3;
  for (int i = 0; i < z.seq_n[v]; ++i) {
    const int s = z.seq_sym[v][i];
    dput(w, pos, z.cl_code[v][s], z.cl_len[v][s]), pos += z.cl_len[v][s];
    const int nx = s == 16 ? 2 : s == 17 ? 3 : s == 18 ? 7 : 0;
    dput(w, pos, z.seq_ext[v][i], nx), pos += nx;
  }
  return pos;
}

// the longest match of position p with the earlier position c, up to maxl bytes
TMH_DDEV int dmatch_len(const uint8_t* raw, int p, int c, int maxl) {
  int l = 0;
  while (l + 4 <= maxl) {  // four bytes at a time (neither side is aligned)
    uint32_t a, b;
    __builtin_memcpy(&a, raw + c + l, 4);
    __builtin_memcpy(&b, raw + p + l, 4);
    if (a != b) return l + (__builtin_ctz(a ^ b) >> 3);
    l += 4;
  }
  while (l < maxl && raw[c + l] == raw[p + l]) ++l;
  return l;
}

// The greedy parse, in order: bit p of z.tok = a token starts at p (z.tok is
// zero on entry).  One walker; on the device the first wave takes 64
// positions' steps into registers at a time and walks the matches among them
// with lane reads (a walk through LDS paid one LDS round trip per token, a
// lane read per literal ~40 cycles of scalar issue: DESIGN §18.4).
TMH_DDEV void dparse(DShared& z, int n, int tid) {
#if defined(__HIP_DEVICE_COMPILE__)
  if (tid >= 64) return;
  int p = 0;  // the next token's position: the same in every lane
  for (int base = 0; base < n; base += 64) {
    const int q = base + tid;
    const int l = q < n ? z.lenb[q] : 0;
    const int step = l ? l + 3 : 1;
    uint64_t mask = 0;
    const int end = base + 64 < n ? base + 64 : n;
    // one step per match taken: the literals up to it are a run of mask bits
    const uint64_t matches = __builtin_amdgcn_ballot_w64(step != 1);
    while (p < end) {
      const int i = __builtin_amdgcn_readfirstlane(p - base);
      const uint64_t rest = matches >> i;
      if (rest == 0) {  // literals to the window's end
        mask |= ~0ull << i;
        p = end;
        break;
      }
      const int t = i + __builtin_ctzll(rest);  // <= 63
      mask |= (~0ull << i) & (~0ull >> (63 - t));
      p = base + t + __builtin_amdgcn_readlane(step, t);
    }
    mask &= end - base < 64 ? (1ull << (end - base)) - 1 : ~0ull;
    if (tid == 0) {
      z.tok[base >> 5] = (uint32_t)mask;
      z.tok[(base >> 5) + 1] = (uint32_t)(mask >> 32);
    }
  }
#else
  if (tid != 0) return;
  int p = 0;
  while (p < n) {
    z.tok[p >> 5] |= 1u << (p & 31);
    const int l = z.lenb[p];
    p += l ? l + 3 : 1;
  }
#endif
}

// One segment (n bytes in z.raw, zero padded) as one block at z.bitpos.
// dist: n uint16 of global scratch (match distance - 1 per position); head:
// the 1 << kDHashBits buckets (position + 1 of the most recent insert).
TMH_DDEV void deflate_segment(DShared& z, int n, int last, uint32_t* w, uint16_t* dist,
                              uint32_t* head, int tid, int nt) {
  for (int i = tid; i < (1 << kDHashBits); i += nt) head[i] = 0;
  for (int i = tid; i < kDSeg / 32; i += nt) z.tok[i] = 0;
  for (int i = tid; i < 288; i += nt) z.hist_ll[0][i] = z.hist_ll[1][i] = (i == 256 ? 1u : 0u);
  for (int i = tid; i < 32; i += nt) z.hist_d[i] = 0;
  TMH_DSYNC_GLOBAL();
  // matches: every position of a batch against the buckets of earlier batches
  for (int b0 = 0; b0 < n; b0 += kDBatch) {
    for (int i = tid; i < kDBatch; i += nt) {
      const int p = b0 + i;
      if (p >= n) continue;
      int best = 0, bestd = 0;
      if (p + kDMinMatch <= n) {
        const int maxl = n - p < kDMaxMatch ? n - p : kDMaxMatch;
        const uint32_t hc = TMH_DLOAD32(&head[dhash4(z.raw + p)]);
        for (int k = 0; k < 4; ++k) {
          const int d = k == 0 ? 1 : k == 1 ? 2 : k == 2 ? 4 : (hc ? p - (int)(hc - 1) : 0);
          if (d <= 0 || d > p || d > 32768) continue;
          const int l = dmatch_len(z.raw, p, p - d, maxl);
          if (l > best || (l == best && d < bestd)) best = l, bestd = d;
          if (best == maxl) break;  // the later candidates are no nearer
        }
        if (best < kDMinMatch) best = 0;
      }
      z.lenb[p] = (uint8_t)(best ? best - 3 : 0);
      dist[p] = (uint16_t)(best ? bestd - 1 : 0);
    }
    TMH_DSYNC();
    for (int i = tid; i < kDBatch; i += nt) {
      const int p = b0 + i;
      if (p + kDMinMatch <= n) TMH_DMAX32(&head[dhash4(z.raw + p)], (uint32_t)(p + 1));
    }
    // the barrier's workgroup fence waits for the atomics to be performed (in
    // L2, where the next batch's TMH_DLOAD32 reads): no wider fence needed
    TMH_DSYNC();
  }
  dparse(z, n, tid);
  TMH_DSYNC_GLOBAL();
  // symbol counts of both dynamic variants
  for (int p = tid; p < n; p += nt) {
    const int x = z.raw[p];
    TMH_DADD32(&z.hist_ll[kDModeLit][x], 1u);
    if ((z.tok[p >> 5] >> (p & 31)) & 1u) {
      const int l = z.lenb[p];
      if (l) {
        int ls, ds, nx;
        uint32_t xv;
        dlen_sym(l + 3, ls, nx, xv);
        ddist_sym((int)dist[p] + 1, ds, nx, xv);
        TMH_DADD32(&z.hist_ll[kDModeMatch][ls], 1u);
        TMH_DADD32(&z.hist_d[ds], 1u);
      } else {
        TMH_DADD32(&z.hist_ll[kDModeMatch][x], 1u);
      }
    }
  }
  dbuild_code(z, z.hist_ll[kDModeMatch], kDLl, 15, z.ll_len[kDModeMatch], tid, nt);
  dbuild_code(z, z.hist_ll[kDModeLit], kDLl, 15, z.ll_len[kDModeLit], tid, nt);
  dbuild_code(z, z.hist_d, kDDist, 15, z.d_len, tid, nt);
  if (tid == 0) {
    drle_header(z, kDModeMatch);
    drle_header(z, kDModeLit);
  }
  dbuild_code(z, z.hist_cl[kDModeMatch], kDCl, 7, z.cl_len[kDModeMatch], tid, nt);
  dbuild_code(z, z.hist_cl[kDModeLit], kDCl, 7, z.cl_len[kDModeLit], tid, nt);
  if (tid == 0) {
    const uint64_t pos = z.bitpos;
    const uint64_t bm = ddyn_bits(z, kDModeMatch), bl = ddyn_bits(z, kDModeLit);
    const uint64_t bs = ((pos + 3 + 7) & ~uint64_t(7)) - pos + 32 + 8 * (uint64_t)n;
    const int mode = bm <= bl && bm <= bs ? kDModeMatch : bl <= bs ? kDModeLit : kDModeStored;
    z.mode = mode;
    uint64_t body;
    if (mode == kDModeStored) {
      dput(w, pos, (uint32_t)last, 3);
      body = (pos + 3 + 7) & ~uint64_t(7);
      dput(w, body, (uint32_t)n, 16);
      dput(w, body + 16, (uint32_t)n ^ 0xFFFFu, 16);
      body += 32;
    } else {
      dassign_codes(z.ll_len[mode], kDLl, z.ll_code[mode]);
      dassign_codes(z.d_len, kDDist, z.d_code);
      dassign_codes(z.cl_len[mode], kDCl, z.cl_code[mode]);
      body = demit_dyn_header(z, mode, w, pos, last);
    }
    z.bitpos = body;
  }
  TMH_DSYNC();
  // the tokens: each thread a run of positions; its bit count, a scan, then the bits
  const int mode = z.mode;
  const int per = (n + nt - 1) / nt;
  const int p0 = tid * per < n ? tid * per : n, p1 = p0 + per < n ? p0 + per : n;
  for (int pass = 0; pass < 2; ++pass) {
    DBitW bw;
    uint32_t bits = 0;
    if (pass) dbw_open(bw, w, z.bitpos + z.part[tid]);
    for (int p = p0; p < p1; ++p) {
      const int x = z.raw[p];
      if (mode == kDModeStored) {
        if (pass) dbw_put(bw, (uint32_t)x, 8);
        bits += 8;
      } else if (mode == kDModeLit) {
        if (pass) dbw_put(bw, z.ll_code[mode][x], z.ll_len[mode][x]);
        bits += z.ll_len[mode][x];
      } else if ((z.tok[p >> 5] >> (p & 31)) & 1u) {
        const int l = z.lenb[p];
        if (l == 0) {
          if (pass) dbw_put(bw, z.ll_code[mode][x], z.ll_len[mode][x]);
          bits += z.ll_len[mode][x];
        } else {
          int ls, ds, lnx, dnx;
          uint32_t lx, dx;
          dlen_sym(l + 3, ls, lnx, lx);
          ddist_sym((int)dist[p] + 1, ds, dnx, dx);
          if (pass) {
            dbw_put(bw, z.ll_code[mode][ls] | lx << z.ll_len[mode][ls], z.ll_len[mode][ls] + lnx);
            dbw_put(bw, z.d_code[ds] | dx << z.d_len[ds], z.d_len[ds] + dnx);
          }
          bits += z.ll_len[mode][ls] + lnx + z.d_len[ds] + dnx;
        }
      }
    }
    if (pass) {
      dbw_close(bw);
    } else {
      z.part[tid] = bits;
      TMH_DSYNC();
      if (tid == 0) {
        uint32_t run = 0;
        for (int t = 0; t < nt; ++t) {
          const uint32_t v = z.part[t];
          z.part[t] = run;
          run += v;
        }
        z.part[nt] = run;
      }
      TMH_DSYNC();
    }
  }
  TMH_DSYNC();
  if (tid == 0) {
    uint64_t pos = z.bitpos + z.part[nt];
    if (mode != kDModeStored) {
      dput(w, pos, z.ll_code[mode][256], z.ll_len[mode][256]);
      pos += z.ll_len[mode][256];
    }
    z.bitpos = pos;
  }
  TMH_DSYNC();
}

TMH_DDEV void dzero_words(uint32_t* w, int64_t words, int tid, int nt) {
  TMH_DSYNC_GLOBAL();
  for (int64_t i = tid; i < words; i += nt) w[i] = 0;
  TMH_DSYNC_GLOBAL();
}

// One chunk: src[0..raw_len) -> one RFC 1950 stream in the slot w (32-bit
// words, deflate_slot_bytes(raw_len) at least); returns its bytes.  dist,
// head: kDSeg uint16 and 1 << kDHashBits uint32 of scratch of this workgroup.
[[maybe_unused]] TMH_DDEV int64_t deflate_chunk(DShared& z, const uint8_t* src, int64_t raw_len, uint32_t* w,
                               uint16_t* dist, uint32_t* head, int tid, int nt) {
  const int64_t slot_words = deflate_slot_bytes(raw_len) / 4;
  dzero_words(w, slot_words, tid, nt);
  if (tid == 0) {
    dput(w, 0, 0x78u | 0x5Eu << 8, 16);  // CM 8, CINFO 7; FLEVEL 1, FCHECK
    z.bitpos = 16;
  }
  const int64_t nseg = raw_len > 0 ? (raw_len + kDSeg - 1) / kDSeg : 1;
  uint64_t sa = 0, sb = 0;  // Adler-32 partial sums of this thread's bytes
  for (int64_t sg = 0; sg < nseg; ++sg) {
    const int64_t s0 = sg * kDSeg;
    const int n = (int)(raw_len - s0 < kDSeg ? raw_len - s0 : kDSeg);
    TMH_DSYNC();
    // 16 bytes per step where the source allows (sums: sum x and sum j x of the group)
    typedef uint32_t DV4 __attribute__((vector_size(16)));
    const int nv = (reinterpret_cast<uintptr_t>(src + s0) & 15) == 0 ? n / 16 : 0;
    for (int i = tid; i < nv; i += nt) {
      const DV4 v = *reinterpret_cast<const DV4*>(src + s0 + 16 * (int64_t)i);
      *reinterpret_cast<DV4*>(z.raw + 16 * i) = v;
      uint32_t g0 = 0, g1 = 0;
      for (int j = 0; j < 16; ++j) {
        const uint32_t x = (v[j >> 2] >> (8 * (j & 3))) & 0xFFu;
        g0 += x;
        g1 += (uint32_t)j * x;
      }
      sa += g0;
      sb += (uint64_t)(raw_len - (s0 + 16 * (int64_t)i)) * g0 - g1;
    }
    for (int i = 16 * nv + tid; i < n + 16; i += nt) {
      const uint8_t x = i < n ? src[s0 + i] : (uint8_t)0;
      z.raw[i] = x;
      sa += x;
      sb += (uint64_t)(raw_len - (s0 + i)) * x;
    }
    TMH_DSYNC();
    deflate_segment(z, n, sg == nseg - 1, w, dist, head, tid, nt);
  }
  z.red[0][tid] = sa % 65521u;
  z.red[1][tid] = sb % 65521u;
  TMH_DSYNC();
  if (tid == 0) {
    uint64_t ta = 0, tb = 0;
    for (int t = 0; t < nt; ++t) ta += z.red[0][t], tb += z.red[1][t];
    const uint64_t a = (1u + ta % 65521u) % 65521u;
    const uint64_t b = ((uint64_t)(raw_len % 65521) + tb % 65521u) % 65521u;
    const uint32_t adler = (uint32_t)((b << 16) | a);
    z.red[0][0] = adler;
    uint64_t pos = (z.bitpos + 7) & ~uint64_t(7);
    for (int i = 0; i < 4; ++i) dput(w, pos, (adler >> (24 - 8 * i)) & 0xFFu, 8), pos += 8;
    z.bitpos = pos;
  }
  TMH_DSYNC();
  const int64_t nblk = raw_len > 0 ? (raw_len + 65534) / 65535 : 1;
  const int64_t stored_len = 2 + 5 * nblk + raw_len + 4;
  if ((int64_t)(z.bitpos >> 3) <= stored_len) return (int64_t)(z.bitpos >> 3);
  // longer than the plain stored stream (many short segments): store the chunk
  const uint32_t adler = (uint32_t)z.red[0][0];
  dzero_words(w, slot_words, tid, nt);
  if (tid == 0) {
    dput(w, 0, 0x78u | 0x5Eu << 8, 16);
    for (int64_t k = 0; k < nblk; ++k) {
      const uint64_t pos = 8 * (uint64_t)(2 + 5 * k + 65535 * k);
      const uint32_t len = (uint32_t)(raw_len - 65535 * k < 65535 ? raw_len - 65535 * k : 65535);
      dput(w, pos, k == nblk - 1 ? 1u : 0u, 8);
      dput(w, pos + 8, len, 16);
      dput(w, pos + 24, len ^ 0xFFFFu, 16);
    }
    uint64_t pos = 8 * (uint64_t)(stored_len - 4);
    for (int i = 0; i < 4; ++i) dput(w, pos, (adler >> (24 - 8 * i)) & 0xFFu, 8), pos += 8;
  }
  for (int64_t i = tid; i < raw_len; i += nt) {
    const int64_t k = i / 65535;
    dput(w, 8 * (uint64_t)(2 + 5 * (k + 1) + i), src[i], 8);
  }
  TMH_DSYNC_GLOBAL();
  return stored_len;
}

// Slot stride in bytes of a piece of at most raw_max bytes (deflate_piece): as
// deflate_slot_bytes, with the sync block's 5 bytes in place of the Adler-32's 4.
TMH_DHD int64_t deflate_piece_slot_bytes(int64_t raw_max) {
  const int64_t nseg = raw_max > 0 ? (raw_max + kDSeg - 1) / kDSeg : 1;
  return ((raw_max + 6 * nseg + 7 + 3) & ~int64_t(3)) + 8;
}

// the all-stored form of a piece: what deflate_piece never exceeds
TMH_DHD int64_t deflate_piece_stored_bytes(int64_t raw_len, int first, int last) {
  const int64_t nblk = raw_len > 0 ? (raw_len + 65534) / 65535 : 1;
  return (first ? 2 : 0) + 5 * nblk + raw_len + (last ? 0 : 5);
}

// One piece of a zlib stream that several workgroups code side by side (PNG:
// png_core.h): src[0..raw_len) coded exactly as deflate_chunk
// codes its segments, but the zlib header only on the `first` piece, BFINAL
// only on the last block of the `last` piece, and no Adler-32.  Every piece but
// the last ends as zlib's Z_SYNC_FLUSH does, with an empty stored block (its
// three header bits, the padding to a byte, 00 00 FF FF), so the pieces are
// whole bytes and the stream is their concatenation.  sums[0], sums[1]: sum x
// and sum (raw_len - i) x_i mod 65521, what the Adler-32 of the whole stream is
// joined from.  A piece longer than its all-stored form is rewritten as that.
// Returns the piece's bytes in the slot w of slot_words words.
[[maybe_unused]] TMH_DDEV int64_t deflate_piece(DShared& z, const uint8_t* src, int64_t raw_len, int first, int last,
                               uint32_t* w, int64_t slot_words, uint16_t* dist, uint32_t* head,
                               uint32_t* sums, int tid, int nt) {
  dzero_words(w, slot_words, tid, nt);
  if (tid == 0) {
    if (first) dput(w, 0, 0x78u | 0x5Eu << 8, 16);
    z.bitpos = first ? 16 : 0;
  }
  const int64_t nseg = raw_len > 0 ? (raw_len + kDSeg - 1) / kDSeg : 1;
  uint64_t sa = 0, sb = 0;
  for (int64_t sg = 0; sg < nseg; ++sg) {
    const int64_t s0 = sg * kDSeg;
    const int n = (int)(raw_len - s0 < kDSeg ? raw_len - s0 : kDSeg);
    TMH_DSYNC();
    typedef uint32_t DV4 __attribute__((vector_size(16)));
    const int nv = (reinterpret_cast<uintptr_t>(src + s0) & 15) == 0 ? n / 16 : 0;
    for (int i = tid; i < nv; i += nt) {
      const DV4 v = *reinterpret_cast<const DV4*>(src + s0 + 16 * (int64_t)i);
      *reinterpret_cast<DV4*>(z.raw + 16 * i) = v;
      uint32_t g0 = 0, g1 = 0;
      for (int j = 0; j < 16; ++j) {
        const uint32_t x = (v[j >> 2] >> (8 * (j & 3))) & 0xFFu;
        g0 += x;
        g1 += (uint32_t)j * x;
      }
      sa += g0;
      sb += (uint64_t)(raw_len - (s0 + 16 * (int64_t)i)) * g0 - g1;
    }
    for (int i = 16 * nv + tid; i < n + 16; i += nt) {
      const uint8_t x = i < n ? src[s0 + i] : (uint8_t)0;
      z.raw[i] = x;
      sa += x;
      sb += (uint64_t)(raw_len - (s0 + i)) * x;
    }
    TMH_DSYNC();
    deflate_segment(z, n, last && sg == nseg - 1, w, dist, head, tid, nt);
  }
  z.red[0][tid] = sa % 65521u;
  z.red[1][tid] = sb % 65521u;
  TMH_DSYNC();
  if (tid == 0) {
    uint64_t ta = 0, tb = 0;
    for (int t = 0; t < nt; ++t) ta += z.red[0][t], tb += z.red[1][t];
    sums[0] = (uint32_t)(ta % 65521u);
    sums[1] = (uint32_t)(tb % 65521u);
    uint64_t pos = z.bitpos;
    if (!last) {  // BFINAL 0, BTYPE 00 are zero bits of the zeroed slot; LEN 0
      pos = (pos + 3 + 7) & ~uint64_t(7);
      dput(w, pos + 16, 0xFFFFu, 16);
      pos += 32;
    }
    z.bitpos = (pos + 7) & ~uint64_t(7);
  }
  TMH_DSYNC();
  const int64_t stored_len = deflate_piece_stored_bytes(raw_len, first, last);
  if ((int64_t)(z.bitpos >> 3) <= stored_len) return (int64_t)(z.bitpos >> 3);
  const int64_t nblk = raw_len > 0 ? (raw_len + 65534) / 65535 : 1;
  const int64_t h = first ? 2 : 0;
  dzero_words(w, slot_words, tid, nt);
  if (tid == 0) {
    if (first) dput(w, 0, 0x78u | 0x5Eu << 8, 16);
    for (int64_t k = 0; k < nblk; ++k) {
      const uint64_t pos = 8 * (uint64_t)(h + 5 * k + 65535 * k);
      const uint32_t len = (uint32_t)(raw_len - 65535 * k < 65535 ? raw_len - 65535 * k : 65535);
      dput(w, pos, last && k == nblk - 1 ? 1u : 0u, 8);
      dput(w, pos + 8, len, 16);
      dput(w, pos + 24, len ^ 0xFFFFu, 16);
    }
    if (!last) dput(w, 8 * (uint64_t)(stored_len - 2), 0xFFFFu, 16);
  }
  for (int64_t i = tid; i < raw_len; i += nt) {
    const int64_t k = i / 65535;
    dput(w, 8 * (uint64_t)(h + 5 * (k + 1) + i), src[i], 8);
  }
  TMH_DSYNC_GLOBAL();
  return stored_len;
}

}  // namespace

}  // namespace tmh
