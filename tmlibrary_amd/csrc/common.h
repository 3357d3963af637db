// Shared definitions for libtmhip (gfx950 / CDNA4 only).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <string>

#include "../../include/tmhip.h"

namespace tmh {

// error plumbing --------------------------------------------------------------
void set_error(const std::string& msg);

struct Error {
  int code;
  std::string msg;
};

#define TMH_HIP(expr)                                                                    \
  do {                                                                                   \
    hipError_t _e = (expr);                                                              \
    if (_e != hipSuccess)                                                                \
      throw ::tmh::Error{TMH_EDEVICE, std::string(#expr) + ": " + hipGetErrorString(_e)}; \
  } while (0)

#define TMH_CHECK(cond, code, msg)                         \
  do {                                                     \
    if (!(cond)) throw ::tmh::Error{(code), (msg)};        \
  } while (0)

// kernel timing (bench/roofline support) ----------------------------------------
// When enabled, every launch of a named kernel is bracketed by a pair of HIP
// events on the stream it runs on; tmh_profile_read sums their durations.
struct ProfScope {
  ProfScope(const char* name, hipStream_t s);
  ~ProfScope();
  const char* name_;
  hipStream_t s_;
  void* slot_;
};

// histogram geometry ------------------------------------------------------------
constexpr int kBins = 65536;      // all uint16 values
constexpr int kLdsBins = 32768;   // bins [0, kLdsBins) counted in LDS (u32)
constexpr int kHiBins = kBins - kLdsBins;  // counted with global atomics
constexpr int kHistThreads = 1024;
constexpr int kBinsPerThread = kBins / kHistThreads;  // 64

// log10 LUT entries staged in LDS by the per-pixel kernels (f64 / f32x2): 32 KB
constexpr int kLutLds = 4096;

// quantile positions (np.percentile 'linear' previous/next sorted positions)
struct QPos {
  const int32_t* lo;  // [Q] previous sorted positions (tables uploaded by the caller)
  const int32_t* hi;  // [Q] next sorted positions
  int Q;
  double scale;  // (Q - 1) / (n - 1): the quantile at a sorted position, up to rounding
  int32_t last;  // n - 1
  int hi_next;   // hi[q] == min(lo[q] + 1, n - 1) for every q: hi is not read
  int64_t tstride;  // order statistics: words between quantile tiles (sites x kOsTile)
};

// Order statistics (per site and quantile, u32 previous | next << 16) are
// stored quantile-tiled, [Q / kOsTile][site][kOsTile]: the ordered percentile
// sum (one thread per quantile, sites in order) then reads a contiguous 1 KB
// run per site per workgroup instead of 1 KB every Q words.  A buffer with
// room for C sites has tile stride C * kOsTile words.
constexpr int kOsTile = 256;
__host__ __device__ inline int64_t os_tiles(int64_t Q) { return (Q + kOsTile - 1) / kOsTile; }

// ---------------------------------------------------------------------------
// f64 refinement of the f32 correction
// ---------------------------------------------------------------------------
// The correct kernels compute 10**t in f32 (log2 domain).  Their result o
// carries a relative error below kRefineK1 * a + kRefineK2 (a = mean(std)/std
// of the pixel; v_log/v_exp 1 ulp, f32 coefficients, fma roundings: derived
// in DESIGN.md §3), so |o_f32 - o_f64| < 1 -- and the truncated uint16 is
// within 1 DN of the reference -- wherever |o| < T = 1 / (K1 * a_max + K2),
// a_max the image's largest finite a.  Pixels with |o| >= T (saturated pixels
// in dim corners: corrected values up to ~1e6 that numpy wraps modulo 2^16)
// are appended to a fixup list by the streaming kernel, and a small kernel
// after it recomputes them in f64, op for op as the reference does.  (Doing
// the f64 work inline would make every streaming kernel reserve its
// registers: the chain pass fell from 8 to 5 waves per SIMD.)
constexpr double kRefineK1 = 6.7e-6;
constexpr double kRefineK2 = 4.2e-6;

// per corrector, device memory: np.mean(std), np.mean(mean) (image.py:627),
// np.log10(1e-10) (the zero pixels' log), T (as double)
struct RefineConst {
  double S, M, zero_log10, T;
};

// pixels to refine, one entry per group of up to 8 consecutive pixels:
// e[i] = site << 40 | mask << 32 | p0 (bit j of mask: pixel p0 + j), for
// i < min(*n, cap); *n > cap means the list overflowed and the fixup
// recomputes every pixel in f64.  (A launch covers < 2^24 sites.)
struct FixList {
  unsigned long long* e;
  unsigned int* n;
  unsigned int cap;
};

__device__ __forceinline__ unsigned long long fix_code8(uint32_t mask, int64_t site, int64_t p0) {
  return ((unsigned long long)site << 40) | ((unsigned long long)(mask & 0xFFu) << 32) |
         (unsigned long long)(uint32_t)p0;
}

__device__ __forceinline__ void fix_push8(const FixList& fl, uint32_t mask, int64_t site, int64_t p0) {
  const unsigned int i = atomicAdd(fl.n, 1u);
  if (i < fl.cap) fl.e[i] = fix_code8(mask, site, p0);
}

__device__ __forceinline__ void fix_push(const FixList& fl, int64_t site, int64_t px) {
  fix_push8(fl, 1u, site, px);
}

// entry i of the list (or, overflowed, the i-th group of 8 pixels)
__device__ __forceinline__ void fix_entry(const FixList& fl, bool all, int64_t i, int64_t npx,
                                          int64_t& site, int64_t& p0, uint32_t& mask) {
  if (all) {
    const int64_t gps = (npx + 7) / 8;  // groups per site
    site = i / gps;
    p0 = (i - site * gps) * 8;
    mask = 0xFFu;
  } else {
    const unsigned long long e = fl.e[i];
    site = (int64_t)(e >> 40);
    mask = (uint32_t)(e >> 32) & 0xFFu;
    p0 = (int64_t)(e & 0xFFFFFFFFull);
  }
}

// ChannelImage._correct_illumination (tmlib/image.py:619-631) of one pixel in
// f64, one rounding per numpy operation; returns the int32 numpy's x86
// astype truncates to (NaN, +-inf, out of range -> INT32_MIN).
template <bool LOG>
__device__ __forceinline__ int32_t correct_ref_f64(uint32_t x, double mean, double std, double S,
                                                   double M, double zero_log10) {
#pragma clang fp contract(off)
  double v = (double)x;
  if (LOG) v = (x == 0u) ? zero_log10 : log10(v);  // img[img == 0] = 1e-10; log10
  double t = (v - mean) / std;
  t = t * S;
  t = t + M;
  if (LOG) t = exp10(t);  // 10 ** img
  return (t > -2147483649.0 && t < 2147483648.0) ? (int32_t)t : INT32_MIN;
}

// 16-byte non-temporal loads and stores: data streamed once (sites in, sites
// out), kept out of L2's way.
typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));
__device__ __forceinline__ uint4 ld_nt(const uint4* p) {
  const u32x4_t v = __builtin_nontemporal_load(reinterpret_cast<const u32x4_t*>(p));
  return make_uint4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ void st_nt(uint4* p, uint4 v) {
  const u32x4_t w = {v.x, v.y, v.z, v.w};
  __builtin_nontemporal_store(w, reinterpret_cast<u32x4_t*>(p));
}
// A site pointer read from a block table is a generic pointer: the compiler
// then emits flat loads (slower than global loads, and counted on both the
// vector-memory and LDS counters).  Site loads through a global-address-space
// pointer stay global_load.
typedef __attribute__((address_space(1))) const u32x4_t gsite_t;
__device__ __forceinline__ gsite_t* to_global(const void* p) { return (gsite_t*)p; }
__device__ __forceinline__ uint4 ld_nt(gsite_t* p) {
  const u32x4_t v = __builtin_nontemporal_load(p);
  return make_uint4(v.x, v.y, v.z, v.w);
}

// launches (defined in the .hip files) -------------------------------------------
// part: optional scratch of part_cap doubles for site-split launches (null: one part)
// forced_parts: 0 = pick the site split automatically, 1..4 = that many parts
// Blocked site layout: the sites of a launch live in blocks of 1 << shift
// consecutive sites each (device arrays of block base pointers; in == null:
// one contiguous run at the launch's in / out pointers).  A block holds a
// multiple of every configuration's sites per unit (shift >= 2).
struct SiteTab {
  const uint16_t* const* in = nullptr;
  uint16_t* const* out = nullptr;
  int shift = 0;
};

// Values beyond the packed fused configuration's LDS slices (>= 16,384 on
// bright sites): appended per site as u16 (staged in LDS, one reservation per
// site and unit) instead of one global atomic each (~61 B of HBM traffic per
// atomic, profiles/r4/abl_rare_atomics_r4ab.jsonl); k_rare_count folds each
// site's list into its histogram.  cnt[s] counts every append; entries past
// cap took the global atomic instead.  v == null: atomics only.
struct RareList {
  uint16_t* v = nullptr;      // site s: v[s * cap, s * cap + min(cnt[s], cap))
  unsigned int* cnt = nullptr;
  unsigned int cap = 0;
};
constexpr int kRareLo = 16384;  // the packed configuration's slice size

// site s of a launch in its layout (contiguous at base, or blocked)
__device__ __forceinline__ int64_t site_block(const SiteTab& t, int64_t s) { return s >> t.shift; }
__device__ __forceinline__ int64_t site_in_block(const SiteTab& t, int64_t s) {
  return s & ((1ll << t.shift) - 1);
}

// bright: 1 = the host's site probe found bright sites (the 20,472-entry LUT
// pass in three site parts where the launch allows), 0 = standard
void launch_welford(const uint16_t* sites, int64_t npx, int64_t n_sites, int64_t n0, double* rn,
                    double* mean, double* m2, const double* lut, int log_transform,
                    double* part, size_t part_cap, int forced_parts,
                    unsigned long long* wide, int bright, hipStream_t s,
                    const SiteTab& tab = SiteTab{});
// Site probe: out[0] = 8-pixel groups sampled (kProbeGroups, spread over the
// launch's first <= 64 sites), out[1] / out[2] = those holding a value >=
// 4,096 / >= 16,384 (device words; the caller copies them to the host)
void launch_site_probe(const uint16_t* sites, int64_t npx, int64_t n_sites, unsigned int* out,
                       hipStream_t s, const SiteTab& tab = SiteTab{});
// vlh: the order statistics of the launch's first site (buffer + site *
// kOsTile) in a buffer with room for vlh_ld sites (kOsTile layout above)
void launch_hist_scatter(const uint16_t* sites, int64_t npx, int64_t n_sites, uint32_t* hist_hi,
                         const QPos& p, uint32_t* vlh, int64_t vlh_ld, unsigned long long* pooled,
                         int64_t* zero_counts, uint32_t* site_hist, hipStream_t s);
// very wide launches: the exact per-site histogram in LDS as u16 pairs from
// one more read of the sites, scanned into order statistics; the pooled
// histogram through pooled_parts, kPooledParts zero-maintained copies of it
// (workgroups spread their adds over them: fewer same-address collisions)
constexpr int kPooledParts = 16;
void launch_hist_site_u16(const uint16_t* sites, int64_t npx, int64_t n_sites, uint32_t* slab,
                          const QPos& p, uint32_t* vlh, int64_t vlh_ld,
                          unsigned long long* pooled, unsigned long long* pooled_parts,
                          int64_t* zero_counts, uint32_t* site_hist, hipStream_t s,
                          const SiteTab& tab = SiteTab{});
void launch_pct_accumulate(const uint32_t* vlh, int64_t n_sites, int64_t vlh_ld, int Q,
                           const double* gamma, double* acc, hipStream_t s);
// quantiles [q_begin, q_begin + q_count) only; acc points at the range
void launch_pct_accumulate_range(const uint32_t* vlh, int64_t n_sites, int64_t vlh_ld, int q_begin,
                                 int q_count, const double* gamma, double* acc, hipStream_t s,
                                 const unsigned long long* only_xwide = nullptr,
                                 unsigned long long xthr = 0);
void launch_finalize(const double* mean, const double* m2, int64_t n, int64_t npx, double* out_mean,
                     double* out_std, hipStream_t s);
// var = M2 / (n - 1), NaN where n < 2 (stats.py:94-102)
void launch_variance(const double* m2, int64_t n, int64_t npx, double* out_var, hipStream_t s);
void launch_merge1(const double* mean, int64_t n, int64_t npx, double* nmean, hipStream_t s);
void launch_merge2(double* mean, const double* m2, int64_t n_r, const double* sum_nmean,
                   int64_t n_total, int64_t npx, double* m2c, hipStream_t s);
void launch_copy_f64(const double* src, double* dst, int64_t n, hipStream_t s);
struct ZeroList {
  unsigned long long* p[8];
  int64_t count[8];  // u64 elements
  int n = 0;
  void add(void* ptr, int64_t elems) {
    TMH_CHECK(n < 8, TMH_EINVAL, "zero list is full");
    p[n] = static_cast<unsigned long long*>(ptr);
    count[n++] = elems;
  }
};
void launch_zero_u64(const ZeroList& z, hipStream_t s);
constexpr int kMaxJobs = 8;          // jobs (a rank's channels) of one multi-job launch
// Small u32 arrays zeroed in one launch (a fused pass's per-job fixup
// counters and unit queues: one kernel, not a fill per array)
struct ZeroList32 {
  static constexpr int kCap = 2 * kMaxJobs;  // two arrays per job
  unsigned int* p[kCap];
  int count[kCap];  // u32 elements
  int n = 0;
  void add(void* ptr, int elems) {
    TMH_CHECK(n < kCap, TMH_EINVAL, "zero list is full");
    p[n] = static_cast<unsigned int*>(ptr);
    count[n++] = elems;
  }
};
void launch_zero_u32(const ZeroList32& z, hipStream_t s);

// Fused jobs' histogram tails: per job the pooled histogram (a column sum of
// the sites' histograms over the rounds the masks name) and every site's
// order statistics, in two launches for all the jobs
struct TailJob {
  uint32_t* hist;                  // the job's histogram slab (zero-maintained)
  unsigned long long* rmask;       // per site: rounds holding counts (zero-maintained)
  const unsigned long long* rm_all;  // the union of the masks, or null
  QPos qp;                         // the handle's quantile table (tstride set)
  uint32_t* vlh;                   // order statistics of the job's first site
  unsigned long long* pooled;
  int64_t* zero_counts;
  uint32_t* site_hist;             // may be null
  int64_t n_sites;
};
struct TailJobs {
  TailJob j[kMaxJobs];
  int n;
};
void launch_hist_finalize_jobs(const TailJobs& J, hipStream_t s);
void launch_hist_finalize(const TailJob& job, hipStream_t s);  // one job
constexpr int kMaxPlanes = 2 * kMaxJobs;
void launch_smooth(const double* in, double* out, double* tmp, int H, int W, const double* d_w,
                   int radius, hipStream_t s);
// np <= kMaxPlanes planes; sq (may be null): per plane 0 = read as is, else
// the plane is M2 read as the finalized std sqrt(M2 / sq) (sq = n - 1; < 0:
// NaN), sigma 5 only
// psum / pmin (may be null): per plane the coefficient tiles' partial sums
// and smallest positive values (k_tile_sums' partition), written as the
// sigma-5 pass stores its outputs, or by k_tile_sums after the two-pass form
void launch_smooth_planes(const double* const* in, double* const* out, double* const* tmp,
                          const double* sq, int np, int H, int W, const double* d_w, int radius,
                          hipStream_t s, double* const* psum, double* const* pmin);
// Coefficient tiles: kSumTH rows x kSumTW columns of a plane (the sigma-5
// smoothing's workgroup tile); a plane's sums are fixed-order sums of its
// tiles' partials (deterministic, whichever kernel made them)
constexpr int kSumTH = 16, kSumTW = 216;
int coef_tiles(int H, int W);
void launch_tile_sums(const double* const* x, double* const* psum, double* const* pmin, int np,
                      int H, int W, hipStream_t s);
void launch_smooth2(const double* in0, const double* in1, double* out0, double* out1,
                    double* tmp0, double* tmp1, int H, int W, const double* d_w, int radius,
                    hipStream_t s);
void launch_build_corr_lut(float2* lut, int log_transform, double zero_log10, hipStream_t s);
// Per job (a corrector) of a coefficient launch: its (smoothed) mean / std
// planes, the reduction scratch (3 x n_partial) and sums (sum(std),
// sum(mean), min positive std), and every coefficient form (coef / coef_lin
// null: left out, launch_coeffs_forms makes them when needed; apply_kernels.hip
// k_coeffs_all: coef (LUT path, mconst = (M hi, M lo, T, 0)), coef2 / coef_lin
// / mconst2 (packed log2-domain path, fused_kernels.hip), coef64 (f64 (mean,
// std) for the refinement) and rc (RefineConst)).
struct CoefJobs {
  const double* mean[kMaxJobs];
  const double* std[kMaxJobs];
  double* partial[kMaxJobs];
  double* sums[kMaxJobs];
  float4* coef[kMaxJobs];
  float2* coef2[kMaxJobs];
  float2* coef_lin[kMaxJobs];
  double2* coef64[kMaxJobs];
  float4* mconst[kMaxJobs];
  float4* mconst2[kMaxJobs];
  RefineConst* rc[kMaxJobs];
  int log_transform[kMaxJobs];
  double zero_log10[kMaxJobs];
};
// partials_ready: J.partial already holds the tiles' sums (the smoothing wrote them)
void launch_coeffs_jobs(const CoefJobs& J, int n_jobs, int H, int W, bool partials_ready,
                        hipStream_t s);
// coef (LUT path) and coef_lin (chain) from coef64 + sums, for a job whose
// coefficient launch left them out (CoefJobs entries null)
void launch_coeffs_forms(const double2* coef64, const double* sums, int64_t npx, int log_transform,
                         float4* coef, float2* coef_lin, hipStream_t s);
// Refinement of the pixels a correct launch flagged (fl), written into out
// (u16 or u8 of in's type, contiguous sites; clip as the launch); launched on
// the same stream.
void launch_fix_correct(const void* in, void* out, int elem_bytes, int64_t npx, int64_t n_sites,
                        const FixList& fl, const double2* coef64, const RefineConst* rc,
                        int log_transform, int clip_lo, int clip_hi, hipStream_t s);
// The fused pass's fixups: one or several uint16 jobs (contiguous or blocked)
// in one launch
struct FixJob {
  const uint16_t* in;
  uint16_t* out;
  int64_t n_sites;
  FixList fl;
  const double2* c64;
  const RefineConst* rc;
  SiteTab tab;
  unsigned long long* wide;  // the job's Welford wide counters to reset, or null
};
struct FixJobs {
  FixJob j[kMaxJobs];
  int n;
};
void launch_fix_correct_jobs(const FixJobs& J, int64_t npx, int log_transform, int clip_lo,
                             int clip_hi, hipStream_t s);
void launch_correct_u16(const uint16_t* in, uint16_t* out, int64_t npx, int64_t n_sites,
                        const float4* coef, const float2* lut, const float4* mconst,
                        const FixList& fl, int log_transform, int clip_lo, int clip_hi,
                        hipStream_t s);
void launch_correct_u8(const uint8_t* in, uint8_t* out, int64_t npx, int64_t n_sites,
                       const float4* coef, const float2* lut, const float4* mconst,
                       const FixList& fl, int log_transform, int clip_lo, int clip_hi,
                       hipStream_t s);
// fused pass configurations (fused_kernels.hip kNarrowCfg, kWideCfg; the
// numbers are the public ones of TMH_OPT_FUSED_CONFIG).  kFusedAuto picks
// per job on the host from the site probe: kFusedNarrow (four sites per unit,
// 4,096-bin slices) unless at least kWideFrac of the probed pixel groups hold
// a value >= 4,096, then kFusedWide: four sites, 16,384 bins each as u16
// counters packed two sites to a word.  The retired shapes 0, 1, 2 and 4 (one
// or two sites per unit, 32,768 u32 bins) lost to these: 17.67-17.75 ms against
// 15.95-16.11 on bright sites (profiles/r3/ab_fused_packed_bright_r3z20.jsonl),
// 22.4 against 18.6 (profiles/r2/mb_fused_bright_r2f.txt).
constexpr int kFusedQueueInts = 16;  // fused pass scratch: 8 unit counters + 64-bit round union
constexpr int kFusedAuto = -1;
constexpr int kFusedNarrow = 3;
constexpr int kFusedWide = 5;
constexpr double kWideFrac = 0.02;
// very wide: a third of the 8-pixel groups hold a value >= 16,384 (~5% of the
// pixels beyond the wide configuration's slices: from there its global atomics
// cost more than one more read of the sites); the fused pass then runs without
// its histogram and k_hist_site_u16 builds the histograms
constexpr double kXWideFrac = 0.33;
// the Welford pass's bright form: >= kBrightFrac of the probed groups hold a
// value >= 4,096
constexpr double kBrightFrac = 0.10;
// the fused pass without its histogram (very wide sites: k_hist_site_u16
// builds the histograms)
constexpr int kFusedNoHist = 100;
// One fused pass over one or several jobs (a rank's channels, same image
// size, configuration and transform): job j's units follow job j-1's in one
// sweep, each unit with its own job's sites, coefficients, histograms, round
// masks and fixup list.  uni: the job's round-mask union (its corrector's
// queues + 8); queues: the launch's kFusedQueueInts unit counters; the caller
// zeroes both on the launch's stream.
struct FusedJob {
  const uint16_t* in;
  uint16_t* out;
  int64_t n_sites;
  const float4* coef;     // coef2 as float4 planes
  const float4* mconst2;
  FixList fl;
  uint32_t* hist;
  unsigned long long* rmask;
  unsigned long long* uni;
  SiteTab tab;
  RareList rl;
};
struct FusedJobs {
  FusedJob j[kMaxJobs];
  int n;
};
// cfg: kFusedNarrow, kFusedWide or kFusedNoHist -- exactly one launch; bands:
// pixel bands of the unit sweep (0: the configuration's, more for a short
// launch -- fused_kernels.hip fused_bands)
void launch_correct_hist(const FusedJobs& J, int64_t npx, int log_transform, int clip_lo,
                         int clip_hi, int* queues, int n_wg, int cfg, int bands, hipStream_t s);
// after launch_correct_hist with a RareList: each site's list into its
// histogram (hist + s * kBins), on the same stream
void launch_rare_count(const RareList& rl, uint32_t* hist, int64_t n_sites, hipStream_t s);
// illuminati chain (chain_kernels.hip)
void launch_align(const void* in, void* out, int elem_bytes, int64_t n_sites, int H, int W, int oh,
                  int ow, const tmh_window* d_win, hipStream_t s);
void launch_map_u8(const uint16_t* in, uint8_t* out, int64_t n, int lo, int hi, hipStream_t s);
// (launches its own fixup kernel after the chain pass; lut8: 64 KB of device
// scratch for the 16-bit clip + scale table, required)
void launch_chain_u8(const uint16_t* in, uint8_t* out, int H, int W, int64_t n_sites,
                     const float2* coef_lin, const float4* mconst2, const FixList& fl,
                     const double2* coef64, const RefineConst* rc, int log_transform,
                     const tmh_window* d_win, int lo, int hi, uint8_t* lut8, hipStream_t s,
                     double zero_log10 = -10.0);
// jterator channel stack (chain_kernels.hip): d_tab = int32 [n_sites * slots]
// plane of each (site, slot) or -1, [n_planes] site, [n_planes] slot,
// [n_planes] windows; coef == null: raw pixels; any_unmapped: some (site, slot)
// has no plane.  Launches its own fixup.
void launch_stack_u16(const uint16_t* in, uint16_t* out, int64_t n_planes, int H, int W,
                      int64_t n_sites, int slots, int out_h, int out_w, const int32_t* d_tab,
                      const float4* coef, const float2* lut, const float4* mconst, const FixList& fl,
                      const double2* coef64, const RefineConst* rc, int log_transform,
                      int any_unmapped, hipStream_t s);
// jterator object tables (objects_kernels.hip)
void launch_label_minmax(const int32_t* planes, int64_t n_planes, int64_t npx, int32_t* d_max,
                         int32_t* d_min, hipStream_t s);
void launch_object_table(const int32_t* planes, int64_t n_planes, int H, int W, int32_t max_label,
                         tmh_object_row* rows, hipStream_t s);
// jterator intensity measurements (measure_kernels.hip): strides in elements of
// elem_bytes (1 or 2) bytes; rows [n_planes][max_label + 1][n_channels];
// out f64 [n_groups][max_label + 1][n_channels][5]
void launch_intensity_table(const int32_t* labels, const void* pixels, int elem_bytes,
                            int64_t n_planes, int H, int W, int n_channels, int64_t cs, int64_t ps,
                            int64_t rs, int64_t xs, int32_t max_label, tmh_intensity_row* rows,
                            hipStream_t s);
void launch_intensity_features(const tmh_intensity_row* rows, int64_t n_planes, int64_t n_groups,
                               int32_t max_label, int n_channels, double* out, hipStream_t s);
// jterator object outlines (contour_kernels.hip): the count pass and scan,
// then the write pass on the same arguments; the scratch lives across both
struct ContourScratch {
  int32_t* lists = nullptr;     // rows whose box fits no LDS form, the large one, the small one
  void* dims = nullptr;
  uint64_t* ws = nullptr;       // their workspace
  int64_t n_rows = 0;
  unsigned long long words = 0, pixels = 0;
  unsigned int n_list[3] = {0u, 0u, 0u};
  ContourScratch() = default;
  ContourScratch(const ContourScratch&) = delete;
  ContourScratch& operator=(const ContourScratch&) = delete;
  ~ContourScratch();
};
void contours_measure(const int32_t* planes, int64_t n_planes, int H, int W, int32_t max_label,
                      const tmh_object_row* rows, tmh_contour_object* objects,
                      ContourScratch& scratch, int64_t* n_contours, int64_t* n_points,
                      hipStream_t s);
void contours_write(const int32_t* planes, int H, int W, int32_t max_label,
                    const tmh_object_row* rows, tmh_contour_object* objects,
                    const ContourScratch& scratch, tmh_contour* contours, int32_t* points,
                    hipStream_t s);
// jterator object input (polygon_kernels.hip): the checks that read the lists
// (TMH_EINVAL by name, nothing written), then the planes zeroed and drawn.
// check: polygons_check_bytes() of device scratch shared by both.
int64_t polygons_check_bytes();
void polygons_check(const int32_t* points, const int64_t* first, const int32_t* plane,
                    int64_t n_polygons, int64_t n_planes, int64_t y_offset, int64_t x_offset,
                    void* check, int64_t* n_points, hipStream_t s);
void polygons_fill(const int32_t* points, const int64_t* first, const int32_t* plane,
                   const int32_t* label, int64_t n_polygons, int64_t n_planes, int H, int W,
                   int64_t y_offset, int64_t x_offset, int32_t* out, void* check, hipStream_t s);
// the clustering tool (cluster_kernels.hip): X is [n][d] f64; cen / scl
// (nullptr: none) are applied as (x - c) / s on load.  cnt[2 d]: per column the
// non-NaN values, then the +-inf values.  The *_chunks functions size the
// partial buffers of the fixed-order sums.
void cluster_census(const double* X, int64_t n, int d, unsigned long long* cnt, hipStream_t s);
int64_t cluster_colsum_chunks(int64_t n);
// out[f] = sum of x (mean == nullptr) or of (x - mean[f])^2 over the column's non-NaN rows / cnt[f]
void cluster_colstat(const double* X, int64_t n, int d, const double* cen, const double* scl,
                     const unsigned long long* cnt, const double* mean, double* part, double* out,
                     hipStream_t s);
int64_t cluster_sum_chunks(int64_t n);
// out[v] = the sum of vec[v][0..n), v < n_vec; part[n_vec * chunks]
void cluster_sum(const double* vec, int64_t n, int n_vec, double* part, double* out, hipStream_t s);
void cluster_robust_scale(const double* X, int64_t n, int d, const double* cen, const double* scl,
                          double* out, hipStream_t s);
// state[d * r][2] = (0, rank); hist[d * r * 256]; out[d * r]
void cluster_select(const double* X, int64_t n, int d, int r, unsigned long long* state,
                    unsigned int* hist, double* out, hipStream_t s);
int64_t cluster_assign_chunks(int64_t n, int d, int k);
// psums[chunks][k][d] / pcounts[chunks][k] (both nullptr: labels only); prev
// and changed are given together or not at all
void cluster_assign(const double* X, int64_t n, int d, int k, const double* cen, const double* scl,
                    const double* centres, const int32_t* prev, int32_t* labels, double* mind,
                    int* changed, double* psums, unsigned int* pcounts, hipStream_t s);
// taken[k]: scratch of the empty-cluster rule
void cluster_update(const double* X, int64_t n, int d, int k, const double* cen, const double* scl,
                    const int32_t* labels, const double* mind, const double* psums,
                    const unsigned int* pcounts, double* sums, long long* counts, const double* old,
                    double* centres_new, double* shift, int64_t* taken, hipStream_t s);
int64_t cluster_seed_blocks(int64_t n);
void cluster_seed_trials(const double* X, int64_t n, int d, int trials, const double* cen,
                         const double* scl, const int64_t* cand, const double* closest, double* out,
                         hipStream_t s);
void cluster_seed_search(const double* closest, int64_t n, int trials, const double* draws,
                         const double* pot, double* block_tot, double* block_excl, double* targets,
                         int64_t* cand, hipStream_t s);
void cluster_seed_pick(const double* pots, int trials, const int64_t* cand, const double* targets,
                       int step, double* pot, int* best, int32_t* indices, double* trace, int tmax,
                       const double* trial_closest, int64_t n, double* closest, hipStream_t s);
void cluster_gather_rows(const double* X, int d, int k, const double* cen, const double* scl,
                         const int32_t* indices, double* centres, hipStream_t s);
// the supervised classification tool (classify_kernels.hip, classify_core.h)
struct ForestNode;
constexpr int64_t kForestLdsBytes = 96 * 1024;  // packed nodes the LDS route stages
// cnt[0] = finite values of X whose f32 cast is infinite
void classify_count_f32_overflow(const double* X, int64_t n, int d, unsigned long long* cnt,
                                 hipStream_t s);
bool forest_fits_lds(int64_t nodes);
int forest_tile_rows(int d, int n_classes, int n_trees);
// proba (nullptr: labels only) [n][n_classes]
void forest_predict(const double* X, int64_t n, int d, int n_classes, int n_trees, int nodes,
                    bool lds_route, const ForestNode* dev_nodes, const int32_t* dev_roots,
                    const double* dev_leaf_value, int32_t* labels, double* proba, hipStream_t s);
// m rows of dev_sv: the support vectors (rbf; dev_coef [k - 1][m], dev_start
// [k + 1]) or the pairs' weight vectors (linear; m = k (k - 1) / 2).  tile_cap
// (0: none) caps the SVs per LDS tile; dec (nullptr: labels only) [n][k (k - 1) / 2]
int svc_tile_svs(int d, int k, int kernel, int m, int cap);
void svc_predict(const double* X, int64_t n, int d, int k, int kernel, double gamma, int m,
                 int tile_cap, const double* cen, const double* scl, const double* dev_sv,
                 const double* dev_coef, const int32_t* dev_start, const double* dev_rho,
                 int32_t* labels, double* dec, hipStream_t s);
// site-image input (inflate_kernels.hip)
int64_t inflate_scratch_bytes(int64_t n_chunks, int64_t raw_max);
void launch_inflate(const uint8_t* src, int64_t src_bytes, const tmh_zchunk* chunks,
                    int64_t n_chunks, int64_t raw_max, uint8_t* dst, int64_t dst_bytes,
                    uint32_t* scratch, int32_t* status, hipStream_t s);
void launch_place_chunks(const uint8_t* raw, const tmh_zchunk* chunks, int64_t n_chunks,
                         int height, int width, int esize, int chunk_rows, int chunk_cols,
                         uint8_t* images, hipStream_t s);
// site-image output (deflate_kernels.hip)
int64_t deflate_bound_bytes(int64_t raw_len);
int64_t deflate_scratch_bytes(int64_t n_chunks, int64_t raw_max);
void launch_gather_chunks(const uint8_t* images, int64_t n_images, int height, int width,
                          int esize, int chunk_rows, int chunk_cols, tmh_zchunk* chunks,
                          uint8_t* raw, hipStream_t s);
void launch_deflate(const uint8_t* raw, int64_t raw_bytes, tmh_zchunk* chunks, int64_t n_chunks,
                    int64_t raw_max, uint8_t* dst, uint8_t* scratch, int32_t* status,
                    int64_t* total, hipStream_t s);
void launch_zproject_max(const void* planes, int64_t n_sites, int z, int height, int width,
                         int esize, void* out, hipStream_t s);
// PNG files of greyscale images (png_kernels.hip): file i at dst + offsets[i],
// offsets[n_images] their total
int64_t png_piece_bytes();
int64_t png_bound_bytes(int height, int width, int esize);
int64_t png_scratch_bytes(int64_t n_images, int height, int width, int esize);
void launch_png(const uint8_t* images, int64_t n_images, int height, int width, int esize,
                uint8_t* dst, int64_t* offsets, uint8_t* scratch, hipStream_t s);
// illuminati tile pyramid (pyramid_kernels.hip); d_tbeg[n_tiles + 1]: tile t's
// rectangles are d_rects[d_tbeg[t], d_tbeg[t + 1])
void launch_tiles_base(const uint8_t* sites, int64_t n_sites, int H, int W,
                       const tmh_tile_rect* d_rects, const int* d_tbeg, uint8_t* tiles,
                       int64_t n_tiles, hipStream_t s);
void launch_pyramid_shrink2(const uint8_t* src, int R, int C, int last_h, int last_w, uint8_t* dst,
                            hipStream_t s);
// JPEG coding of a tile-major level (jpeg_kernels.hip).  tables: the call's
// JpegTables (jpeg_core.h), jpeg_tables_bytes() bytes, built by
// jpeg_tables_host and uploaded by the caller.  measure: offsets[n + 1] = the
// exclusive scan of the files' sizes; write: every file at out + offsets[t].
size_t jpeg_tables_bytes();
void jpeg_tables_host(int quality, void* tables);
void launch_jpeg_measure(const uint8_t* level, int rows, int cols, int last_h, int last_w,
                         const void* d_tables, int64_t* offsets, hipStream_t s);
void launch_jpeg_write(const uint8_t* level, int rows, int cols, int last_h, int last_w,
                       const void* d_tables, const int64_t* offsets, uint8_t* out, hipStream_t s);
// JPEG decoding (jpeg_decode_kernels.hip).  roundtrip: every tile of a level as
// libjpeg decodes it from the file launch_jpeg_write writes for it at `quality`
// (out: the same layout, distinct from level).  decode_tiles: n files at
// blob + offsets[t] into tile storage, dims[n][2] and status[n]; d_tables:
// jpeg_decode_tables_bytes() bytes built by jpeg_decode_tables_host.
void launch_jpeg_roundtrip(const uint8_t* level, int rows, int cols, int last_h, int last_w,
                           int quality, uint8_t* out, hipStream_t s);
size_t jpeg_decode_tables_bytes();
void jpeg_decode_tables_host(void* tables);
void launch_jpeg_decode_tiles(const uint8_t* blob, const int64_t* offsets, int64_t n,
                              const void* d_tables, uint8_t* tiles, int32_t* dims,
                              int32_t* status, hipStream_t s);
// Registration (register_kernels.hip): shifts of n targets against their
// references by FFT cross-correlation; dev_plane (may be NULL): the f32 planes
// [n][H][W].  Returns when the host outputs are filled.
int64_t register_scratch_bytes(int64_t n, int64_t m, int H, int W);
void launch_register(const void* dev_targets, int64_t n, const void* dev_refs, int64_t m, int H,
                     int W, int elem_bytes, const int32_t* host_ref_of, void* dev_scratch,
                     int64_t scratch_bytes, int32_t* host_y, int32_t* host_x, float* host_peak,
                     float* dev_plane, hipStream_t s);
void launch_clip_u16(const uint16_t* in, uint16_t* out, int64_t n, int lo, int hi, hipStream_t s);
void launch_synth(uint16_t* out, int64_t n_sites, int H, int W, uint64_t seed, int channel,
                  int64_t first_site, int dist, hipStream_t s);
void synth_tables_host(int dist, int H, int W, int32_t* ln, int32_t* nz, int32_t* ey, int32_t* ex);
// box probe (bench support, synth_kernels.hip): write = copy the sites to the
// output blocks, else read them; clk[4] = (clock64, wall_clock64) at workgroup
// 0's start and end
void launch_box_probe(const uint16_t* const* in_blocks, uint16_t* const* out_blocks, int shift,
                      int64_t n_sites, int64_t npx, int write, unsigned long long* clk,
                      unsigned int* sink, int n_cus, hipStream_t s);
// the flat shape: one 16-byte group per thread over one contiguous run of sites
void launch_box_probe_flat(const uint16_t* in, uint16_t* out, int64_t n_sites, int64_t npx,
                           int write, unsigned int* sink, hipStream_t s);

__host__ __device__ inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

}  // namespace tmh
