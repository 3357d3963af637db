// illuminati post-correct chain (gfx950 / MI355X): SURVEY.md §8(f) rank 3.
//
// Reference: tmlib/workflow/illuminati/api.py:396-405 takes every corrected
// site through
//   image.correct(stats)            tmlib/image.py:633-670
//        .align(crop=False)         tmlib/image.py:345-454  (shift + zero pad)
//        .clip(clip_min, clip_max)  tmlib/image.py:570-597
//        .scale(clip_min, clip_max) tmlib/image.py:493-568  (uint16 -> uint8 LUT)
// before cutting pyramid tiles.  k_chain_u8t (any width: k_chain_u8_scalar)
// does all four in one pass that reads the uint16 site (2 B/px) and writes the
// uint8 tile source (1 B/px); k_fix_chain then refines in f64 the few pixels
// whose f32 value is not safe to truncate.
//
// align is a window copy: the host evaluates the reference's numpy slicing
// into (src_r0, src_c0, dst_r0, dst_c0, rows, cols); output pixels outside
// the destination window are 0, which clip/scale map to scale8(clip_min) = 0.
//
// scale is the reference's LUT
//   zeros(lo) | linspace(0, 255, hi - lo).astype(uint16) | 255 * ones(65536 - hi)
// evaluated per pixel the way numpy builds it: entry lo + i is
// trunc(double(i) * (255.0 / (n - 1))) with n = hi - lo, except the last one
// (i = n - 1), which linspace sets to exactly 255, and n = 1 (a lone 0).  One
// f64 multiply, bit-identical to the table (pinned exhaustively against the
// reference's LUTs, tests/golden/map_uint8.npz).  k_chain_lut8 evaluates it
// once per launch for all 65,536 values, clip included.
#include "common.h"
#include "correct_core.h"

namespace tmh {

__device__ __forceinline__ uint32_t scale8(uint32_t v, int lo, int hi, double step) {
  if (v < (uint32_t)lo) return 0u;
  if (v >= (uint32_t)hi) return 255u;
  const int n = hi - lo, i = (int)v - lo;
  if (n == 1) return 0u;
  if (i == n - 1) return 255u;
  return (uint32_t)((double)i * step);  // x in [0, 255): trunc == astype(uint16)
}

__device__ __forceinline__ bool in_window(int r, int c, const tmh_window& w) {
  return (unsigned)(r - w.dst_r0) < (unsigned)w.rows && (unsigned)(c - w.dst_c0) < (unsigned)w.cols;
}

// align (any dtype): out[n][oh][ow], window per site
template <typename T>
__global__ void k_align(const T* __restrict__ in, T* __restrict__ out, int H, int W, int oh, int ow,
                        const tmh_window* __restrict__ win) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t s = blockIdx.y;
  if (i >= (int64_t)oh * ow) return;
  const tmh_window w = win[s];
  const int r = (int)(i / ow), c = (int)(i % ow);
  T v = (T)0;
  if (in_window(r, c, w))
    v = in[s * (int64_t)H * W + (int64_t)(r - w.dst_r0 + w.src_r0) * W + (c - w.dst_c0 + w.src_c0)];
  out[s * (int64_t)oh * ow + i] = v;
}

__global__ void k_map_u8(const uint16_t* __restrict__ in, uint8_t* __restrict__ out, int64_t n,
                         int lo, int hi, double step) {  // no clip: the LUT's zeros / 255 tails
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = (uint8_t)scale8(in[i], lo, hi, step);
}

// Clip to [lo, hi] then the reference LUT, branch-free: T = n - 1 for
// n = hi - lo > 1 (linspace's end point and v = hi give 255), T = 1 for n = 1.
__device__ __forceinline__ uint32_t clip_scale8(uint32_t v16, int lo, int hi, int T, double step) {
  const uint32_t v = min(max(v16, (uint32_t)lo), (uint32_t)hi);
  const uint32_t i = v - (uint32_t)lo;
  return i >= (uint32_t)T ? 255u : (uint32_t)((double)i * step);
}

// one pixel px (site s, source index p) of the packed-f32 correction; m =
// mconst2 (M' hi, M' lo, zf, T): beyond T the pixel is flagged for the f64
// refinement (common.h, k_fix_chain)
template <bool LOG>
__device__ __forceinline__ uint32_t correct16(uint32_t px, float mu, float a, const float4 m,
                                              int64_t s, int64_t p, const FixList& fl) {
  float L = (float)px;
  if (LOG) L = __builtin_amdgcn_logf(__builtin_fmaxf(L, m.z));
  const float t = fmaf(L - mu, a, m.x);
  float o = LOG ? __builtin_amdgcn_exp2f(t) : t;
  if (__builtin_fabsf(o) >= m.w) fix_push(fl, s, p);
  o = __builtin_fminf(o, 2147418112.0f);  // >= 2^31, inf, NaN -> low half 0 (x86 astype)
  if (!LOG) o = __builtin_fmaxf(o, -2147483648.0f);
  return (uint32_t)(int32_t)o & 0xFFFFu;
}

// n < 8 bytes of v (low first) at the 8-aligned address p: dword, short, byte
// pieces, each naturally aligned
__device__ __forceinline__ void store_head(uint8_t* p, uint64_t v, int n) {
  if (n & 4) {
    *reinterpret_cast<uint32_t*>(p) = (uint32_t)v;
    p += 4;
    v >>= 32;
  }
  if (n & 2) {
    *reinterpret_cast<uint16_t*>(p) = (uint16_t)v;
    p += 2;
    v >>= 16;
  }
  if (n & 1) *p = (uint8_t)v;
}

// the low n < 8 bytes of v ending just below the 8-aligned address end
__device__ __forceinline__ void store_tail(uint8_t* end, uint64_t v, int n) {
  uint8_t* p = end - n;
  if (n & 1) {
    *p = (uint8_t)v;
    p += 1;
    v >>= 8;
  }
  if (n & 2) {
    *reinterpret_cast<uint16_t*>(p) = (uint16_t)v;
    p += 2;
    v >>= 16;
  }
  if (n & 4) *reinterpret_cast<uint32_t*>(p) = (uint32_t)v;
}

// blockIdx -> tile with XCD x (= blockIdx % 8, the dispatch round-robin)
// owning tiles [x*q + min(x, r), ...) of n = 8q + r: a bijection on [0, n)
__device__ __forceinline__ int64_t xcd_tile(int64_t b, int64_t n) {
  const int64_t q = n / 8, r = n % 8, x = b % 8, k = b / 8;
  return x * q + (x < r ? x : r) + k;
}

typedef float f32x2c_t __attribute__((ext_vector_type(2)));

// The chain pass for W % 8 == 0, source-driven: one thread = 8 consecutive
// SOURCE pixels (one 16-byte load per site), their coefficients loaded once
// and reused for every site of its part (blockIdx.y = site part).  align is a
// flat shift per site, off = (dst_r0 - src_r0) * W + (dst_c0 - src_c0): source
// pixel p lands at p + off, a bijection onto [off, npx + off), and source
// pixels outside the window land outside the destination window (they write
// the padding value, 0 scaled).  The destinations no source pixel reaches,
// [0, off) or [npx + off, npx), are padded by the first / last workgroup.
//
// clip + scale is one byte load: the reference's table for every 16-bit value
// (k_chain_lut8, 64 KB) is copied into LDS and indexed by the cast's low half.
// Workgroups have kChainThreads = 1,024 threads, two per CU beside the table
// (smaller ones copy it too often: 256 threads ran 37 ms, 512 21.6, 1,024 14.6,
// profiles/r2/mb_chain_lut64_r2lt.txt).
//
// The pass is VALU-bound (~24 issue slots per pixel, two of them quarter-rate
// transcendentals), so the per-pixel work is trimmed:
//  * a group is flagged for k_fix_chain when its max |o| passes the f32 error
//    bound of its largest a, |o| (K1 a_max8 + K2) >= 1 (the fused pass's
//    per-pixel rule, fcorrect8, with the group's largest a), and k_fix_chain
//    refines only the pixels beyond their own bound (the launch-wide T =
//    1 / (K1 a_max + K2) with whole groups refined ran 0.30 ms of f64 fixups
//    per 3,456 bench sites);
//  * no min/max before the cast: every |o| >= 1 / K2 (< 2^18) fails its own
//    f32 bound and is refined in f64; the pixels that keep their streamed byte
//    have |o| < 0.998 / K2 < 2^18 -- there v_cvt_i32_f32 truncates exactly as
//    the x86 cast does, so no clamp is needed; NaN converts to 0 on both;
//  * ZADD: a zero pixel's floor as x + zf instead of max(x, zf) -- two pixels
//    per v_pk_add_f32; exact for zf < 2^-25 (x >= 1 plus zf rounds to x);
//  * the table bytes packed with v_perm (3 per 4 bytes) instead of shifts,
//    ors and a masking bitop;
//  * the align window's byte mask only for threads whose 8 pixels are not all
//    inside it (a divergent branch: whole waves skip it).
//
// The 8 result bytes of thread i go to [8i + off, 8i + off + 8).  With off a
// multiple of the 128-B line they are stored directly.  Otherwise a shifted
// run written lane by lane would split every wave's store across one more,
// partial line on each side, so runs are first made 8-byte aligned with the
// upper lane's bytes (wave shuffle), the lines a wave covers alone are stored
// as aligned 8-byte words, and the lines two waves (or two workgroups) share
// -- the seams -- are assembled in LDS and stored as whole 16-B chunks.
// Workgroups follow xcd_tile's order: neighbouring tiles' shifted outputs
// share a line at their seam, and a seam inside one XCD's L2 merges instead of
// leaving two partial lines to write back.
constexpr int kChainThreads = 1024;
template <bool LOG, bool ZADD>
__global__ __launch_bounds__(kChainThreads) __attribute__((amdgpu_waves_per_eu(8))) void k_chain_u8t(
    const uint16_t* __restrict__ in, uint8_t* __restrict__ out, int H, int W, int64_t n_sites,
    int64_t per, const float2* __restrict__ coef_lin, const float4* __restrict__ mconst2,
    FixList fl, const tmh_window* __restrict__ win, const uint8_t* __restrict__ lut8) {
  constexpr int NT = kChainThreads;
  extern __shared__ __attribute__((aligned(16))) uint8_t slut[];
  for (int i = threadIdx.x; i < 65536 / 16; i += NT)
    reinterpret_cast<uint4*>(slut)[i] = reinterpret_cast<const uint4*>(lut8)[i];
  __syncthreads();
  const int64_t npx = (int64_t)H * W;
  const int64_t ngroups = npx >> 3;
  const int64_t tile = xcd_tile(blockIdx.x, gridDim.x);
  const int64_t g = tile * NT + threadIdx.x;
  const bool live = g < ngroups;
  const int lane = threadIdx.x & 63;
  // two sets of seam lines used in turn: one barrier per site
  constexpr int kSeams = NT / 64 + 1;  // seam s = line L0 + 512 s
  __shared__ __attribute__((aligned(16))) uint8_t stage[2 * kSeams * 128];
  const int64_t p0 = (live ? g : 0) * 8;
  const int r = (int)(p0 / W), c0 = (int)(p0 % W);
  const float4 m = mconst2[0];
  const f32x2c_t M = {m.x, m.x};
  const f32x2c_t Z = {m.z, m.z};
  f32x2c_t mu[4], a[4];
  float thr;  // this thread's flag threshold on max |o| (below)
  {
    const float4* cf = reinterpret_cast<const float4*>(coef_lin + p0);
    float am = 0.0f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float4 v0 = live ? cf[k] : make_float4(0.f, 1.f, 0.f, 1.f);
      mu[k] = (f32x2c_t){v0.x, v0.z};
      a[k] = (f32x2c_t){v0.y, v0.w};
      am = __builtin_fmaxf(am, __builtin_fmaxf(__builtin_fabsf(v0.y), __builtin_fabsf(v0.w)));
    }
    // the fused pass's per-pixel bound |o| (K1 a + K2) >= 0.998 (fcorrect8),
    // taken with the largest a of the thread's 8 pixels: max |o| >= thr flags
    // the group (a superset of the pixels the per-pixel bound flags)
    constexpr float K1 = (float)(kRefineK1 * 1.002), K2 = (float)(kRefineK2 * 1.002);
    thr = 0.998f / __builtin_fmaf(am, K1, K2);
  }
  const int64_t s0 = (int64_t)blockIdx.y * per;
  const int64_t s1 = s0 + per < n_sites ? s0 + per : n_sites;
  const uint4* src = reinterpret_cast<const uint4*>(in) + (live ? g : 0);

  auto site = [&](const uint4 cur, const int64_t s) {
    const tmh_window w = win[s];  // uniform: scalar loads
    const uint32_t wd[4] = {cur.x, cur.y, cur.z, cur.w};
    f32x2c_t t[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      t[k].x = (float)(wd[k] & 0xFFFFu);
      t[k].y = (float)(wd[k] >> 16);
    }
    if (LOG) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (ZADD) {
          t[k] += Z;
        } else {
          t[k].x = __builtin_fmaxf(t[k].x, m.z);
          t[k].y = __builtin_fmaxf(t[k].y, m.z);
        }
        t[k].x = __builtin_amdgcn_logf(t[k].x);
        t[k].y = __builtin_amdgcn_logf(t[k].y);
      }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) t[k] = __builtin_elementwise_fma(t[k] - mu[k], a[k], M);
    float mx = 0.0f;  // largest |result| of the 8 pixels (v_max3 with |.| modifiers)
    uint32_t o[8];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const float x = LOG ? __builtin_amdgcn_exp2f(t[k][h]) : t[k][h];
        mx = __builtin_fmaxf(mx, __builtin_fabsf(x));
        o[2 * k + h] = slut[(uint32_t)(int32_t)x & 0xFFFFu];
      }
    }
    // bytes (o0, o1, o2, o3): v_perm pairs, then the pairs' low halves -- in
    // the loads' basic block, where the compiler knows the bytes are
    // zero-extended (sunk past the branch below it masks each byte first)
    uint32_t lo4 = __builtin_amdgcn_perm(__builtin_amdgcn_perm(o[3], o[2], 0x0c0c0400u),
                                         __builtin_amdgcn_perm(o[1], o[0], 0x0c0c0400u), 0x05040100u);
    uint32_t hi4 = __builtin_amdgcn_perm(__builtin_amdgcn_perm(o[7], o[6], 0x0c0c0400u),
                                         __builtin_amdgcn_perm(o[5], o[4], 0x0c0c0400u), 0x05040100u);
    asm volatile("" : "+v"(lo4), "+v"(hi4));  // keeps the packing here (no code is emitted)
    // rare: a group beyond its f32 bound is flagged for the f64 refinement
    if (mx >= thr && live) fix_push8(fl, 0xFFu, s, p0);
    // pixels outside the source window write the padding value (0 after
    // clip/scale); only threads with a pixel outside build the byte mask
    const int cs = c0 - w.src_c0;
    const bool inside = w.cols >= 8 && (unsigned)(r - w.src_r0) < (unsigned)w.rows &&
                        (unsigned)cs <= (unsigned)(w.cols - 8);
    if (!inside) {
      int jlo = -cs < 0 ? 0 : (-cs > 8 ? 8 : -cs);
      int jhi = w.cols - cs < 0 ? 0 : (w.cols - cs > 8 ? 8 : w.cols - cs);
      if ((unsigned)(r - w.src_r0) >= (unsigned)w.rows) jhi = 0;
      const uint64_t keep = jhi > jlo ? ((~0ull >> (8 * (8 - (jhi - jlo)))) << (8 * jlo)) : 0ull;
      lo4 &= (uint32_t)keep;
      hi4 &= (uint32_t)(keep >> 32);
    }
    const uint64_t v8 = ((uint64_t)hi4 << 32) | lo4;
    // byte offsets inside one site fit in 32 bits (the launch checks npx < 2^30)
    const int n32 = (int)npx;
    const int off = (w.dst_r0 - w.src_r0) * W + (w.dst_c0 - w.src_c0);  // uniform
    const int D = (int)p0 + off;  // destination of byte 0
    const int rr = off & 7;       // uniform
    uint8_t* o8 = out + s * npx;
    // the destinations no source pixel reaches -- [0, off) for off > 0,
    // [npx + off, npx) for off < 0, all outside the destination window -- take
    // the padding value, written by the site part's first / last workgroup
    if ((off > 0 && tile == 0) || (off < 0 && tile == (int64_t)gridDim.x - 1)) {
      const int b0 = off > 0 ? 0 : n32 + off, b1 = off > 0 ? off : n32;
      const uint8_t pad = slut[0];
#pragma unroll 1
      for (int b = b0 + (int)threadIdx.x; b < b1; b += NT) o8[b] = pad;
    }
    if ((off & 127) == 0) {  // line-aligned destination: direct stores
      if (live && (unsigned)D < (unsigned)n32) *reinterpret_cast<uint64_t*>(o8 + D) = v8;
      return;
    }
    // A wave's 512 output bytes [o0 + 512 w, +512) fully cover the three
    // lines L0 + 512 w + 128 k (k = 1..3): its lanes store their aligned
    // 8-byte words there directly.  The lines L0 + 512 s (s = 0..16) are
    // shared with the neighbouring wave (or workgroup): their words and the
    // partial words at the waves' edges go to an LDS copy of those lines,
    // stored after one barrier as whole 16-B chunks.
    const int o0 = (int)(tile * NT * 8) + off;  // uniform: destination of thread 0's byte 0
    const int L0 = o0 & ~127;                   // its line (floor, also for o0 < 0)
    uint8_t* seam = stage + (int)(s & 1) * (kSeams * 128);
    const uint32_t nlo = (uint32_t)__shfl_down((int)lo4, 1, 64);
    const uint32_t nhi = (uint32_t)__shfl_down((int)hi4, 1, 64);
    const uint64_t n8 = ((uint64_t)nhi << 32) | nlo;
    const bool wtop = lane == 63 || g + 1 >= ngroups;  // no upper neighbour in the wave
    if (live) {
      const int X = rr == 0 ? D : D - rr + 8;  // the aligned word this lane completes
      const int r = X - L0;
      const bool in_seam = (r & 511) < 128;
      uint8_t* sp = seam + (r >> 9) * 128 + (r & 127);
      if (rr == 0 || !wtop) {  // a whole word: ours, or our [8 - rr, 8) + the upper lane's [0, 8 - rr)
        const uint64_t v = rr == 0 ? v8 : (v8 >> (8 * (8 - rr))) | (n8 << (8 * rr));
        if (in_seam)
          *reinterpret_cast<uint64_t*>(sp) = v;
        else if ((unsigned)X < (unsigned)n32)
          *reinterpret_cast<uint64_t*>(o8 + X) = v;
      } else {  // the wave's top lane: only our bytes of that word
        if (in_seam)
          store_head(sp, v8 >> (8 * (8 - rr)), rr);
        else if ((unsigned)X < (unsigned)n32)
          store_head(o8 + X, v8 >> (8 * (8 - rr)), rr);
      }
      if (rr != 0 && lane == 0) {  // our bytes [0, 8 - rr): the top of word X - 8, a seam line
        const int q = X - 8 - L0;
        store_tail(seam + (q >> 9) * 128 + (q & 127) + 8, v8, 8 - rr);
      }
    }
    __syncthreads();  // seam lines complete (the other set was read before it)
    // valid destination bytes of this workgroup: [v0, v1) (uniform; the last
    // workgroup may own fewer groups)
    const int wg_bytes = (int)((ngroups - tile * NT < NT ? ngroups - tile * NT : NT) * 8);
    const int v0 = o0 > 0 ? o0 : 0;
    const int v1 = o0 + wg_bytes < n32 ? o0 + wg_bytes : n32;
    if ((int)threadIdx.x < kSeams * 8) {
      const int sl = threadIdx.x >> 3, ch = threadIdx.x & 7;
      const int c = L0 + 512 * sl + 16 * ch;
      const uint8_t* src8 = seam + sl * 128 + 16 * ch;
      if (c + 16 <= v1 && c >= v0) {
        *reinterpret_cast<uint4*>(o8 + c) = *reinterpret_cast<const uint4*>(src8);
      } else if (c < v1 && c + 16 > v0) {
        for (int b = 0; b < 16; ++b)
          if (c + b >= v0 && c + b < v1) o8[c + b] = src8[b];
      }
    }
  };

  // The next site's load is issued before this site's processing, and
  // unconditionally (the last iteration reloads its own site): a load under a
  // condition in the loop compiles to a full wait for the load just issued.
  // The 32 waves of a CU hide the rest of the latency.  (A pipeline that keeps
  // several sites' loads in flight ran slower for this shape: 19.4 vs 14.5
  // ms, profiles/r3/mb_chain_pipeline_r3n.txt.)
  if (s0 >= s1) return;
  uint4 nxt = ld_nt(src + s0 * ngroups);
  for (int64_t s = s0; s < s1; ++s) {
    const uint4 cur = nxt;
    nxt = ld_nt(src + (s + 1 < s1 ? s + 1 : s) * ngroups);
    site(cur, s);
  }
}

// The 16-bit clip + scale table of k_chain_u8t: entry v = scale8(clip(v)).
__global__ void k_chain_lut8(uint8_t* __restrict__ lut8, int lo, int hi, int T, double step) {
  const int v = (int)blockIdx.x * 256 + threadIdx.x;
  if (v < 65536) lut8[v] = (uint8_t)clip_scale8((uint32_t)v, lo, hi, T, step);
}

// Any width: one thread per output pixel.
template <bool LOG>
__global__ __launch_bounds__(256) void k_chain_u8_scalar(const uint16_t* __restrict__ in,
                                                          uint8_t* __restrict__ out, int H, int W,
                                                          int64_t n_sites,
                                                          const float2* __restrict__ coef_lin,
                                                          const float4* __restrict__ mconst2,
                                                          FixList fl,
                                                          const tmh_window* __restrict__ win,
                                                          int lo, int hi, int T, double step) {
  const int64_t npx = (int64_t)H * W;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= npx) return;
  const int r = (int)(i / W), c = (int)(i % W);
  const float4 m = mconst2[0];
  for (int64_t s = 0; s < n_sites; ++s) {
    const tmh_window w = win[s];
    uint32_t v = clip_scale8(0u, lo, hi, T, step);
    if (in_window(r, c, w)) {
      const int64_t p = (int64_t)(r - w.dst_r0 + w.src_r0) * W + (c - w.dst_c0 + w.src_c0);
      const float2 k = coef_lin[p];
      v = clip_scale8(correct16<LOG>(in[s * npx + p], k.x, k.y, m, s, p, fl), lo, hi, T, step);
    }
    out[s * npx + i] = (uint8_t)v;
  }
}

// f64 refinement of the chain pixels the pass flagged (FixList, common.h;
// source pixels): the corrected value -> clip -> scale, written at the pixel's
// aligned destination; pixels outside the source window were written as
// padding and are left alone.  Overflowed list: every source pixel.
// A pixel of a flagged group whose f32 value (recomputed with the streaming
// kernels' own instructions) lies within its error bound |o| (K1 a + K2) <
// 0.998 keeps the byte the streaming kernel wrote; the others are refined.
template <bool LOG>
__global__ __launch_bounds__(256) void k_fix_chain(const uint16_t* __restrict__ in,
                                                   uint8_t* __restrict__ out, int H, int W,
                                                   int64_t n_sites, FixList fl,
                                                   const double2* __restrict__ c64,
                                                   const RefineConst* __restrict__ rc,
                                                   const tmh_window* __restrict__ win, int lo,
                                                   int hi, int T, double step,
                                                   const float2* __restrict__ coef_lin,
                                                   const float4* __restrict__ mconst2) {
  const int64_t npx = (int64_t)H * W;
  const unsigned int n = *fl.n;
  const bool all = n > fl.cap;
  const int64_t total = all ? n_sites * ((npx + 7) / 8) : (int64_t)n;
  if (total == 0) return;
  const RefineConst k = *rc;
  // one thread per (entry, pixel): the 8 lanes of an entry read its pixels
  // and coefficients together, and the rare f64 refinements spread over lanes
  for (int64_t it = (int64_t)blockIdx.x * 256 + threadIdx.x; it < total * 8;
       it += (int64_t)gridDim.x * 256) {
    const int64_t i = it >> 3;
    const int j = (int)(it & 7);
    int64_t s, p0;
    uint32_t mask;
    fix_entry(fl, all, i, npx, s, p0, mask);
    {
      const int64_t p = p0 + j;
      if (!((mask >> j) & 1u) || p >= npx) continue;
      const tmh_window w = win[s];
      const int r = (int)(p / W), c = (int)(p - (int64_t)r * W);
      if ((unsigned)(r - w.src_r0) >= (unsigned)w.rows ||
          (unsigned)(c - w.src_c0) >= (unsigned)w.cols)
        continue;
      const uint16_t px = in[s * npx + p];
      {  // the streaming kernels' f32 value and its bound
        constexpr float K1 = (float)(kRefineK1 * 1.002), K2 = (float)(kRefineK2 * 1.002);
        const float4 m = mconst2[0];
        const float2 cf = coef_lin[p];
        float L = (float)px;
        if (LOG) L = __builtin_amdgcn_logf(__builtin_fmaxf(L, m.z));
        const float t = __builtin_fmaf(L - cf.x, cf.y, m.x);
        const float o = LOG ? __builtin_amdgcn_exp2f(t) : t;
        if (__builtin_fabsf(o) * __builtin_fmaf(cf.y, K1, K2) < 0.998f) continue;
      }
      const double2 q = c64[p];
      const uint32_t v16 =
          (uint32_t)correct_ref_f64<LOG>(px, q.x, q.y, k.S, k.M, k.zero_log10) & 0xFFFFu;
      const int64_t d = (int64_t)(r - w.src_r0 + w.dst_r0) * W + (c - w.src_c0 + w.dst_c0);
      out[s * npx + d] = (uint8_t)clip_scale8(v16, lo, hi, T, step);
    }
  }
}

// ---------------------------------------------------------------------------
// jterator channel stack (tmlib/workflow/jterator/api.py:283-316)
// ---------------------------------------------------------------------------
// Every plane (z-plane x time point) of a site's channel is corrected, cropped
// to its crop=True alignment window and written to slot zplane * n_tpoints +
// tpoint of the site's [out_h][out_w][slots] stack.  In the general form
// (k_stack_px) threads own OUTPUT pixels: a thread gathers the pixel's `slots`
// source values (one per plane, each a coalesced 2-byte-per-lane row read) and
// writes them together, so the interleaved stack leaves as one contiguous run
// per wave; a (site, slot) no plane maps to is written as 0 by the same thread
// (np.zeros).  Its grid has the site on the fast axis (blockIdx.x) and the
// pixel chunk on the slow one, so the workgroups in flight together work on the
// same region of different sites and their coefficient reads (16 B per pixel
// against 2 B of site data; windows of different sites are a few pixels apart)
// meet in L2.  slots == 1, the common case, has two forms of its own with
// 16-byte loads and stores: a copy (k_stack_copy8) and, corrected, a
// source-driven pass that keeps the coefficients in registers (k_stack_src8).
// The arithmetic is k_correct_u16_vec8's (correct_core.h), no clip; flagged
// pixels go to the same f64 refinement list, keyed by plane and SOURCE pixel,
// and k_fix_stack writes them at their stack position.
struct StackTab {
  const int32_t* plane_of;  // [n_sites * slots]: the plane mapped to (site, slot), or -1
  const int32_t* site_of;   // [n_planes]
  const int32_t* slot_of;   // [n_planes]
  const tmh_window* win;    // [n_planes]
};

// 8 uint16 at a 2-byte-aligned address
struct __attribute__((packed, aligned(2))) U16x8 {
  uint32_t w[4];
};

constexpr int kStackChunks = 8;  // 256-thread chunks per workgroup: one LDS LUT fill serves them all

// slots == 1, not corrected, out_w % 8 == 0: a thread copies 8 consecutive
// pixels of one output row -- one 16-byte load at the source row's 2-byte
// alignment (src_c0 is arbitrary), one 16-byte store.
__global__ __launch_bounds__(256) void k_stack_copy8(const uint16_t* __restrict__ in,
                                                     uint16_t* __restrict__ out, int H, int W,
                                                     int out_h, int out_w, StackTab tab) {
  const int64_t site = blockIdx.x;
  const int64_t ngroups = ((int64_t)out_h * out_w) >> 3;
  const int plane = tab.plane_of[site];
  uint4* dst = reinterpret_cast<uint4*>(out + site * (int64_t)out_h * out_w);
  const int64_t g0 = (int64_t)blockIdx.y * (kStackChunks * 256) + threadIdx.x;
  tmh_window w = {0, 0, 0, 0, 0, 0};
  if (plane >= 0) w = tab.win[plane];
  const uint16_t* src = in + (plane < 0 ? 0 : plane) * (int64_t)H * W;
  for (int k = 0; k < kStackChunks; ++k) {
    const int64_t g = g0 + k * 256;
    if (g >= ngroups) break;
    uint4 res = make_uint4(0u, 0u, 0u, 0u);
    if (plane >= 0) {
      const int64_t o = g * 8;
      const int r = (int)(o / out_w), c = (int)(o - (int64_t)r * out_w);
      const U16x8 v =
          *reinterpret_cast<const U16x8*>(src + (int64_t)(w.src_r0 + r) * W + (w.src_c0 + c));
      res = make_uint4(v.w[0], v.w[1], v.w[2], v.w[3]);
    }
    dst[g] = res;
  }
}

// slots == 1, corrected, W % 8 == 0: SOURCE-driven, the shape of
// k_correct_u16_vec8.  A thread owns 8 consecutive source pixels of one row,
// loads their coefficients once (16 B a pixel against 2 B of site data) and
// walks the planes: each plane's 16 aligned bytes are corrected and stored at
// the group's place in that plane's site, (r - src_r0, c - src_c0) -- 16 bytes
// at the output row's 2-byte alignment, or pixel by pixel where the group
// straddles the window's left or right edge; groups outside a plane's window
// store nothing.  An output-driven form (coefficients gathered per plane at the
// window's offset) measured 1.5-1.7 ms for 64 sites of 2160 x 2560 against
// 0.4 ms for the plain correction of the same sites.  Sites without a plane
// are zeroed by the same launch (any_unmapped), output group g by thread g.
template <bool LOG>
__global__ __launch_bounds__(256) void k_stack_src8(const uint16_t* __restrict__ in,
                                                    uint16_t* __restrict__ out, int H, int W,
                                                    int out_h, int out_w, int64_t n_planes,
                                                    int64_t n_sites, int any_unmapped,
                                                    StackTab tab, const float4* __restrict__ coef,
                                                    const float2* __restrict__ lut,
                                                    const float4* __restrict__ mconst, FixList fl) {
  __shared__ float2 slut[LOG ? kLutLds : 1];
  if (LOG) {
    for (int i = threadIdx.x; i < kLutLds; i += 256) slut[i] = lut[i];
    __syncthreads();
  }
  const int64_t npx = (int64_t)H * W, ngroups = npx >> 3, opx = (int64_t)out_h * out_w;
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (any_unmapped) {
    const int64_t o = g * 8;  // opx <= npx: the source groups cover every output group
    for (int64_t s = 0; s < n_sites; ++s) {
      if (tab.plane_of[s] >= 0) continue;  // uniform
      uint16_t* d = out + s * opx;
      if (o + 8 <= opx) {
        *reinterpret_cast<U16x8*>(d + o) = U16x8{{0u, 0u, 0u, 0u}};
      } else {
        for (int64_t k = o; k < opx; ++k) d[k] = 0;
      }
    }
  }
  if (g >= ngroups) return;
  const int64_t p0 = g * 8;
  const int r = (int)(p0 / W), c0 = (int)(p0 - (int64_t)r * W);
  const float4 m = mconst[0];
  float4 c[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) c[k] = coef[p0 + k];
  const uint4* src = reinterpret_cast<const uint4*>(in) + g;
  uint4 nxt = n_planes > 0 ? src[0] : make_uint4(0u, 0u, 0u, 0u);
  for (int64_t p = 0; p < n_planes; ++p) {
    const uint4 v = nxt;
    nxt = src[(p + 1 < n_planes ? p + 1 : p) * ngroups];  // the next plane's load in flight
    const tmh_window w = tab.win[p];                       // uniform: scalar loads
    const int rr = r - w.src_r0, cs = c0 - w.src_c0;       // the group's output row, first column
    const int jlo = cs < 0 ? -cs : 0, jhi = out_w - cs < 8 ? out_w - cs : 8;
    if ((unsigned)rr >= (unsigned)out_h || jhi <= jlo) continue;
    const uint32_t u[8] = {v.x & 0xFFFFu, v.x >> 16, v.y & 0xFFFFu, v.y >> 16,
                           v.z & 0xFFFFu, v.z >> 16, v.w & 0xFFFFu, v.w >> 16};
    uint32_t q[8];
#pragma unroll
    for (int j = 0; j < 8; ++j)
      q[j] = correct1<LOG, 16>(u[j], c[j], slut, m, p, p0 + j, fl, -1, 0);
    uint16_t* d = out + (int64_t)tab.site_of[p] * opx + (int64_t)rr * out_w + cs;
    if (jlo == 0 && jhi == 8) {
      *reinterpret_cast<U16x8*>(d) = U16x8{{q[0] | (q[1] << 16), q[2] | (q[3] << 16),
                                            q[4] | (q[5] << 16), q[6] | (q[7] << 16)}};
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (j >= jlo && j < jhi) d[j] = (uint16_t)q[j];
    }
  }
}

// Any slots, any width: a thread owns one output pixel and its `slots`
// adjacent values.  S = 2 / 4: the values leave as one 4- / 8-byte store (the
// pixel's run is that aligned); S = 0: `slots` at run time, 2-byte stores
// (adjacent lanes' runs are adjacent, so a wave still writes one contiguous
// span).
template <bool CORR, bool LOG, int S>
__global__ __launch_bounds__(256) void k_stack_px(const uint16_t* __restrict__ in,
                                                  uint16_t* __restrict__ out, int H, int W,
                                                  int out_h, int out_w, int slots, StackTab tab,
                                                  const float4* __restrict__ coef,
                                                  const float2* __restrict__ lut,
                                                  const float4* __restrict__ mconst, FixList fl) {
  __shared__ float2 slut[CORR && LOG ? kLutLds : 1];
  if (CORR && LOG) {
    for (int i = threadIdx.x; i < kLutLds; i += 256) slut[i] = lut[i];
    __syncthreads();
  }
  const int64_t site = blockIdx.x;
  const int64_t opx = (int64_t)out_h * out_w;
  const int64_t npx = (int64_t)H * W;
  const int ns = S ? S : slots;
  const int32_t* pl = tab.plane_of + site * ns;
  uint16_t* dst = out + site * opx * ns;
  float4 m = make_float4(0.f, 0.f, 0.f, 0.f);
  if (CORR) m = mconst[0];
  auto value = [&](int plane, int r, int c) -> uint32_t {
    if (plane < 0) return 0u;
    const tmh_window w = tab.win[plane];  // uniform per workgroup
    const int64_t sp = (int64_t)(w.src_r0 + r) * W + (w.src_c0 + c);
    const uint32_t u = in[plane * npx + sp];
    if (!CORR) return u;
    return correct1<LOG, 16>(u, coef[sp], slut, m, plane, sp, fl, -1, 0);
  };
  for (int k = 0; k < kStackChunks; ++k) {
    const int64_t o = (int64_t)blockIdx.y * (kStackChunks * 256) + k * 256 + threadIdx.x;
    if (o >= opx) break;
    const int r = (int)(o / out_w), c = (int)(o - (int64_t)r * out_w);
    if (S == 2) {
      const uint32_t a = value(pl[0], r, c), b = value(pl[1], r, c);
      reinterpret_cast<uint32_t*>(dst)[o] = a | (b << 16);
    } else if (S == 4) {
      const uint32_t a = value(pl[0], r, c), b = value(pl[1], r, c);
      const uint32_t d = value(pl[2], r, c), e = value(pl[3], r, c);
      reinterpret_cast<uint2*>(dst)[o] = make_uint2(a | (b << 16), d | (e << 16));
    } else {
      for (int t = 0; t < ns; ++t) dst[o * ns + t] = (uint16_t)value(pl[t], r, c);
    }
  }
}

// f64 refinement of the stack pixels the pass flagged (entries: plane, source
// pixel), written at their (site, row, column, slot); list overflowed: every
// source pixel of every plane.  Pixels outside the plane's window have no
// stack position.
template <bool LOG>
__global__ __launch_bounds__(256) void k_fix_stack(const uint16_t* __restrict__ in,
                                                   uint16_t* __restrict__ out, int H, int W,
                                                   int out_h, int out_w, int slots,
                                                   int64_t n_planes, StackTab tab, FixList fl,
                                                   const double2* __restrict__ c64,
                                                   const RefineConst* __restrict__ rc) {
  const int64_t npx = (int64_t)H * W;
  const unsigned int n = *fl.n;
  const bool all = n > fl.cap;
  const int64_t total = all ? n_planes * ((npx + 7) / 8) : (int64_t)n;
  if (total == 0) return;
  const RefineConst k = *rc;
  for (int64_t it = (int64_t)blockIdx.x * 256 + threadIdx.x; it < total * 8;
       it += (int64_t)gridDim.x * 256) {
    const int64_t i = it >> 3;
    const int j = (int)(it & 7);
    int64_t pln, p0;
    uint32_t mask;
    fix_entry(fl, all, i, npx, pln, p0, mask);
    const int64_t p = p0 + j;
    if (!((mask >> j) & 1u) || p >= npx) continue;
    const tmh_window w = tab.win[pln];
    const int r = (int)(p / W), c = (int)(p - (int64_t)r * W);
    if ((unsigned)(r - w.src_r0) >= (unsigned)out_h || (unsigned)(c - w.src_c0) >= (unsigned)out_w)
      continue;
    const double2 q = c64[p];
    const uint32_t v =
        (uint32_t)correct_ref_f64<LOG>(in[pln * npx + p], q.x, q.y, k.S, k.M, k.zero_log10) & 0xFFFFu;
    const int64_t d = ((int64_t)tab.site_of[pln] * out_h + (r - w.src_r0)) * out_w + (c - w.src_c0);
    out[d * slots + tab.slot_of[pln]] = (uint16_t)v;
  }
}

// d_tab: int32 device table [n_sites * slots | n_planes | n_planes | 6 * n_planes]
// (plane_of, site_of, slot_of, windows); coef == null: the channel is not
// corrected; any_unmapped: some (site, slot) has no plane
void launch_stack_u16(const uint16_t* in, uint16_t* out, int64_t n_planes, int H, int W,
                      int64_t n_sites, int slots, int out_h, int out_w, const int32_t* d_tab,
                      const float4* coef, const float2* lut, const float4* mconst, const FixList& fl,
                      const double2* coef64, const RefineConst* rc, int log_transform,
                      int any_unmapped, hipStream_t s) {
  const int64_t opx = (int64_t)out_h * out_w;
  if (n_sites <= 0 || opx == 0) return;
  ProfScope prof("stack", s);
  StackTab tab;
  tab.plane_of = d_tab;
  tab.site_of = d_tab + n_sites * slots;
  tab.slot_of = tab.site_of + n_planes;
  tab.win = reinterpret_cast<const tmh_window*>(tab.slot_of + n_planes);
  const bool corr = coef != nullptr;
  const int mode = !corr ? 0 : (log_transform ? 2 : 1);
  const dim3 block(256);
  const bool src8 =
      corr && slots == 1 && (W & 7) == 0 && (reinterpret_cast<uintptr_t>(in) & 15) == 0;
  const bool copy8 = !corr && slots == 1 && (out_w & 7) == 0 &&
                     (reinterpret_cast<uintptr_t>(out) & 15) == 0;
  if (src8) {
    const dim3 grid((unsigned)cdiv(((int64_t)H * W) >> 3, 256));
    if (log_transform)
      hipLaunchKernelGGL(k_stack_src8<true>, grid, block, 0, s, in, out, H, W, out_h, out_w,
                         n_planes, n_sites, any_unmapped, tab, coef, lut, mconst, fl);
    else
      hipLaunchKernelGGL(k_stack_src8<false>, grid, block, 0, s, in, out, H, W, out_h, out_w,
                         n_planes, n_sites, any_unmapped, tab, coef, lut, mconst, fl);
  } else if (copy8) {
    const dim3 grid((unsigned)n_sites, (unsigned)cdiv(opx >> 3, kStackChunks * 256));
    hipLaunchKernelGGL(k_stack_copy8, grid, block, 0, s, in, out, H, W, out_h, out_w, tab);
  } else {
    const dim3 grid((unsigned)n_sites, (unsigned)cdiv(opx, kStackChunks * 256));
    const bool a4 = (reinterpret_cast<uintptr_t>(out) & 7) == 0;
    const int S = (slots == 2 && a4) ? 2 : (slots == 4 && a4) ? 4 : 0;
#define TMH_STACK_P(C_, L_, S_)                                                                  \
  hipLaunchKernelGGL((k_stack_px<C_, L_, S_>), grid, block, 0, s, in, out, H, W, out_h, out_w,   \
                     slots, tab, coef, lut, mconst, fl)
#define TMH_STACK_PS(C_, L_)            \
  do {                                  \
    if (S == 2) TMH_STACK_P(C_, L_, 2); \
    else if (S == 4) TMH_STACK_P(C_, L_, 4); \
    else TMH_STACK_P(C_, L_, 0);        \
  } while (0)
    if (mode == 0) TMH_STACK_PS(false, false);
    else if (mode == 1) TMH_STACK_PS(true, false);
    else TMH_STACK_PS(true, true);
#undef TMH_STACK_PS
#undef TMH_STACK_P
  }
  if (corr) {
    if (log_transform)
      hipLaunchKernelGGL(k_fix_stack<true>, dim3(512), block, 0, s, in, out, H, W, out_h, out_w,
                         slots, n_planes, tab, fl, coef64, rc);
    else
      hipLaunchKernelGGL(k_fix_stack<false>, dim3(512), block, 0, s, in, out, H, W, out_h, out_w,
                         slots, n_planes, tab, fl, coef64, rc);
  }
  TMH_HIP(hipGetLastError());
}

double scale_step(int lo, int hi) { return hi - lo > 1 ? 255.0 / (double)(hi - lo - 1) : 0.0; }

void launch_align(const void* in, void* out, int elem_bytes, int64_t n_sites, int H, int W, int oh,
                  int ow, const tmh_window* d_win, hipStream_t s) {
  if (n_sites <= 0 || (int64_t)oh * ow == 0) return;
  const dim3 grid((unsigned)cdiv((int64_t)oh * ow, 256), (unsigned)n_sites);
  if (elem_bytes == 2)
    hipLaunchKernelGGL(k_align<uint16_t>, grid, dim3(256), 0, s, (const uint16_t*)in,
                       (uint16_t*)out, H, W, oh, ow, d_win);
  else
    hipLaunchKernelGGL(k_align<uint8_t>, grid, dim3(256), 0, s, (const uint8_t*)in, (uint8_t*)out,
                       H, W, oh, ow, d_win);
  TMH_HIP(hipGetLastError());
}

void launch_map_u8(const uint16_t* in, uint8_t* out, int64_t n, int lo, int hi, hipStream_t s) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_map_u8, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, s, in, out, n, lo, hi,
                     scale_step(lo, hi));
  TMH_HIP(hipGetLastError());
}

void launch_chain_u8(const uint16_t* in, uint8_t* out, int H, int W, int64_t n_sites,
                     const float2* coef_lin, const float4* mconst2, const FixList& fl,
                     const double2* coef64, const RefineConst* rc, int log_transform,
                     const tmh_window* d_win, int lo, int hi, uint8_t* lut8, hipStream_t s,
                     double zero_log10) {
  if (n_sites <= 0) return;
  TMH_CHECK(lut8 != nullptr, TMH_EINVAL, "launch_chain_u8: no table scratch");
  ProfScope prof("chain", s);
  const int64_t npx = (int64_t)H * W;
  const double step = scale_step(lo, hi);
  const int T = hi - lo > 1 ? hi - lo - 1 : 1;
  const bool vec = (W & 7) == 0 && (reinterpret_cast<uintptr_t>(in) & 15) == 0 &&
                   (reinterpret_cast<uintptr_t>(out) & 7) == 0 && npx < ((int64_t)1 << 30);
  if (vec) {
    hipLaunchKernelGGL(k_chain_lut8, dim3(256), dim3(256), 0, s, lut8, lo, hi, T, step);
    // site parts even out the dispatch rounds (each thread streams its part):
    // 16 parts ran 3,456 sites of 2160x2560 in 12.49 ms against 12.77 with 8
    // (tools/mb/mb_chain.hip)
    const int64_t parts = n_sites >= 128 ? 16 : n_sites >= 64 ? 8 : 1;
    const int64_t per = cdiv(n_sites, parts);
    const dim3 grid((unsigned)cdiv(npx >> 3, kChainThreads), (unsigned)cdiv(n_sites, per));
#define TMH_CHAIN_T(L_, Z_)                                                                      \
  hipLaunchKernelGGL((k_chain_u8t<L_, Z_>), grid, dim3(kChainThreads), 65536, s, in, out, H, W, \
                     n_sites, per, coef_lin, mconst2, fl, d_win, lut8)
    // zf = 10**zero_log10 below 2^-25 (~2.98e-8): the floor as an add is exact
    if (!log_transform) TMH_CHAIN_T(false, false);
    else if (zero_log10 <= -8.0) TMH_CHAIN_T(true, true);
    else TMH_CHAIN_T(true, false);
#undef TMH_CHAIN_T
  } else {
    const dim3 grid((unsigned)cdiv(npx, 256));
    if (log_transform)
      hipLaunchKernelGGL(k_chain_u8_scalar<true>, grid, dim3(256), 0, s, in, out, H, W, n_sites,
                         coef_lin, mconst2, fl, d_win, lo, hi, T, step);
    else
      hipLaunchKernelGGL(k_chain_u8_scalar<false>, grid, dim3(256), 0, s, in, out, H, W, n_sites,
                         coef_lin, mconst2, fl, d_win, lo, hi, T, step);
  }
  if (log_transform)
    hipLaunchKernelGGL(k_fix_chain<true>, dim3(2048), dim3(256), 0, s, in, out, H, W, n_sites, fl,
                       coef64, rc, d_win, lo, hi, T, step, coef_lin, mconst2);
  else
    hipLaunchKernelGGL(k_fix_chain<false>, dim3(2048), dim3(256), 0, s, in, out, H, W, n_sites,
                       fl, coef64, rc, d_win, lo, hi, T, step, coef_lin, mconst2);
  TMH_HIP(hipGetLastError());
}

}  // namespace tmh
