// Internals shared by the abi_*.hip sources of the C-ABI (include/tmhip.h):
// included by them only, not installed.
#pragma once

#include <algorithm>
#include <vector>

#include "common.h"

#pragma GCC visibility push(hidden)  // nothing here is part of the library's interface

namespace tmh {

// every entry point's body runs in one: a thrown Error becomes its code, its
// text tmh_last_error's (abi_core.hip)
template <typename F>
inline int guard(F&& f) {
  try {
    f();
    return TMH_OK;
  } catch (const Error& e) {
    set_error(e.msg);
    return e.code;
  } catch (const std::bad_alloc&) {
    set_error("host allocation failed");
    return TMH_ENOMEM;
  } catch (...) {
    set_error("unknown error");
    return TMH_EDEVICE;
  }
}

// device buffers
template <typename T>
struct DBuf {
  T* p = nullptr;
  size_t n = 0;
  void alloc(size_t count, bool zero = false) {
    release();
    if (count == 0) return;
    if (hipMalloc(&p, count * sizeof(T)) != hipSuccess) {
      p = nullptr;
      throw Error{TMH_ENOMEM, "hipMalloc of " + std::to_string(count * sizeof(T)) + " bytes failed"};
    }
    n = count;
    if (zero) {
      // null-stream memset: our launches run on non-blocking streams, so wait
      TMH_HIP(hipMemset(p, 0, count * sizeof(T)));
      TMH_HIP(hipDeviceSynchronize());
    }
  }
  void ensure(size_t count, bool zero = false) {
    if (count > n) alloc(count, zero);
  }
  // the unpipelined host-buffer entry points: allocate + blocking copy in, blocking copy out
  void upload(const void* host, size_t count) {
    alloc(count);
    TMH_HIP(hipMemcpy(p, host, count * sizeof(T), hipMemcpyHostToDevice));
  }
  void download(void* host, size_t count) const {
    TMH_HIP(hipMemcpy(host, p, count * sizeof(T), hipMemcpyDeviceToHost));
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    n = 0;
  }
  ~DBuf() { release(); }
};

// host staging of the host-buffer entry points (tmh_stats_update,
// tmh_correct_u16): two device slots and two pinned host slots per direction,
// copy streams separate from the compute stream, so the copies of chunk k
// overlap the kernels (and, for correct, the opposite-direction copy) of
// chunk k-1 instead of alternating copy -> kernel -> synchronize.
struct PinBuf {
  void* p = nullptr;
  size_t n = 0;
  void ensure(size_t bytes) {
    if (bytes <= n) return;
    release();
    if (hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) {
      p = nullptr;
      throw Error{TMH_ENOMEM, "hipHostMalloc of " + std::to_string(bytes) + " bytes failed"};
    }
    n = bytes;
  }
  void release() {
    if (p) (void)hipHostFree(p);
    p = nullptr;
    n = 0;
  }
  ~PinBuf() { release(); }
};

// memcpy between pageable and pinned host memory on up to max_t threads (abi_core.hip)
void par_copy(void* dst, const void* src, size_t bytes, int max_t);

// Staging of the host-buffer entry points.  Measured on MI355X boxes
// (tools/diag_host.py, bench extras.host_path): the runtime's own pageable H2D
// path already reaches ~56 GB/s, above a pinned bounce fed by 8 host threads,
// so inputs go straight from the caller's buffer; outputs land in pinned slots
// and are copied out by copy_threads threads, which also spreads the
// first-touch page faults of a fresh numpy output.
struct HostOpts {
  int copy_threads = 8;
  bool set(int option, int value) {
    if (option != TMH_OPT_COPY_THREADS) return false;
    TMH_CHECK(value >= 1 && value <= 64, TMH_EINVAL, "copy threads must be 1..64");
    copy_threads = value;
    return true;
  }
};

struct HostPipe {
  PinBuf out[2];
  hipStream_t h2d = nullptr, d2h = nullptr;
  hipEvent_t ev_in[2]{}, ev_kern[2]{}, ev_done[2]{};
  bool busy[2] = {false, false};
  int64_t s0[2] = {0, 0}, ns[2] = {0, 0};
  void init() {
    if (h2d) return;
    TMH_HIP(hipStreamCreateWithFlags(&h2d, hipStreamNonBlocking));
    TMH_HIP(hipStreamCreateWithFlags(&d2h, hipStreamNonBlocking));
    for (int i = 0; i < 2; ++i) {
      TMH_HIP(hipEventCreateWithFlags(&ev_in[i], hipEventDisableTiming));
      TMH_HIP(hipEventCreateWithFlags(&ev_kern[i], hipEventDisableTiming));
      TMH_HIP(hipEventCreateWithFlags(&ev_done[i], hipEventDisableTiming));
    }
  }
  // after an error mid-call: let queued work finish, forget the chunks (their
  // host destinations belong to the failed call)
  void abandon(hipStream_t compute) {
    if (h2d) (void)hipStreamSynchronize(h2d);
    if (d2h) (void)hipStreamSynchronize(d2h);
    if (compute) (void)hipStreamSynchronize(compute);
    busy[0] = busy[1] = false;
  }
  ~HostPipe() {
    if (!h2d) return;
    (void)hipStreamSynchronize(h2d);
    (void)hipStreamSynchronize(d2h);
    for (int i = 0; i < 2; ++i) {
      (void)hipEventDestroy(ev_in[i]);
      (void)hipEventDestroy(ev_kern[i]);
      (void)hipEventDestroy(ev_done[i]);
    }
    (void)hipStreamDestroy(h2d);
    (void)hipStreamDestroy(d2h);
  }
};

}  // namespace tmh

using namespace tmh;  // as every abi_*.hip source does

struct tmh_stats {
  int device = 0;
  int H = 0, W = 0;
  int64_t npx = 0;
  int Q = 0;
  double scale = 0.0;
  unsigned flags = 0;
  int64_t batch_cap = 0;
  hipStream_t own_stream = nullptr;
  hipStream_t stream = nullptr;
  hipStream_t side = nullptr;   // histogram pass runs here, concurrent with Welford
  // the fused pass's histogram tail when the pass runs on another stream
  // (correct_hist_dev).  (At the lowest priority, with the caller's streams
  // above it, a two-jobs-in-flight bench ran 4-6% slower: profiles/r4/
  // ab_jobs_in_flight_priority_r4y.txt.)
  hipStream_t tail = nullptr;
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  hipEvent_t ev_in = nullptr, ev_out = nullptr;  // ordering against a caller's stream
  // work on other streams the handle's stream must wait for, joined lazily
  // (hstream): a wait enqueued at once would sit in the stream's hardware
  // queue ahead of unrelated work of every stream sharing that queue until
  // the awaited pass had finished
  static constexpr int kJoins = 8;
  hipEvent_t join_ev[kJoins]{};
  hipStream_t join_s[kJoins]{};  // one entry per stream: a later record supersedes
  int join_n = 0;
  int fused_cfg = kFusedAuto;     // TMH_OPT_FUSED_CONFIG (-1: per launch, on the device)
  int wf_parts = 0;               // TMH_OPT_WELFORD_PARTS (0: automatic)
  HostOpts host;                  // TMH_OPT_COPY_THREADS
  bool hist_dirty = false;        // a fused launch may have left counts / round masks behind
  int64_t n = 0;              // sites accumulated (Welford count)
  int64_t n_deferred = 0;     // sites whose order statistics are stored
  int64_t last_batch = 0;
  int64_t pending = 0;        // Welford-updated sites whose histograms are still to come
  DBuf<unsigned long long> wide;  // pixel groups with a value >= 4,096 / >= 16,384 in the pending sites
  // The job's site probe (k_site_probe, first Welford launch after a reset):
  // 8-pixel groups sampled, those with a value >= 4,096, >= 16,384.  The host
  // reads the counts once per job and launches only the Welford pass and the
  // fused configuration they call for (stats_choice).
  DBuf<unsigned int> probe;
  unsigned int* probe_host = nullptr;  // pinned copy
  hipEvent_t ev_probe = nullptr;
  bool probed = false;
  bool probe_queued = false;  // tmh_stats_probe_device: launched, not yet read
  unsigned int probe_cnt[3] = {0u, 0u, 0u};
  int64_t wide_sites = 0;         // sites that count covers
  bool pct_sum_external = false;
  DBuf<double> mean, m2, lut_log, gamma, acc, tmp_mean, tmp_std, rn;
  DBuf<double> wf_part;  // partial (mean, M2) planes of site-split Welford launches
  DBuf<int32_t> q_lo, q_hi;
  DBuf<unsigned long long> pooled, pooled_parts;  // parts: kPooledParts zero-maintained copies
  DBuf<uint32_t> hist_hi, site_hist, hist_full;
  DBuf<unsigned long long> hist_rmask;  // per site: touched high rounds of hist_full
  DBuf<uint16_t> rare_v;                // fused pass, packed configuration: per-site rare lists
  DBuf<unsigned int> rare_n;
  QPos qp{};
  DBuf<uint16_t> stage;  // two device slots of batch_cap sites
  HostPipe pipe;
  DBuf<uint32_t> vlh;  // order statistics (previous | next << 16), quantile-tiled (common.h)
  int64_t vlh_cap = 0;   // deferred mode: sites the tiles have room for
  int64_t vlh_ld = 0;    // tile stride in sites of the current contents
  DBuf<int64_t> zeros;
};

struct tmh_corrector {
  int device = 0;
  int H = 0, W = 0;
  int64_t npx = 0;
  int log_transform = 1;
  double zero_log10 = -10.0;
  hipStream_t stream = nullptr;
  DBuf<float4> coef, mconst, mconst2;
  DBuf<float2> lut, coef2, coef_lin;
  DBuf<double2> coef64;              // f64 (mean, std): the refinement's operands
  DBuf<RefineConst> rc;
  DBuf<unsigned long long> fix_e;    // pixels flagged for the f64 refinement (common.h)
  DBuf<unsigned int> fix_n;
  DBuf<tmh_window> win;  // per-site alignment windows of the chain pass
  DBuf<uint8_t> lut8;    // the chain pass's 16-bit clip + scale table (64 KB)
  int n_wg = 256;
  int bands = 0;     // TMH_OPT_FUSED_BANDS (0: automatic)
  bool forms_stale = false;  // coef / coef_lin not made since the last coefficient update
  DBuf<int> queues;  // fused pass: per-XCD unit counters (dynamic deal)
  DBuf<double> sums, partial;
  DBuf<uint16_t> stage_in, stage_out;
  DBuf<uint8_t> stage8_in, stage8_out;
  HostPipe pipe;
  HostOpts host;  // TMH_OPT_COPY_THREADS
  // a histogram tail still reading queues (round masks) on a statistics
  // handle's stream (correct_hist_dev, cross-stream calls)
  hipEvent_t ev_tail = nullptr;
  bool tail_pending = false;
};

namespace tmh {

inline hipStream_t pick(hipStream_t own, void* s) { return s ? (hipStream_t)s : own; }

// The handle's stream for new work: first it waits for the work on other
// streams joined since its last use (defer_join).
inline hipStream_t hstream(tmh_stats* h) {
  for (int i = 0; i < h->join_n; ++i) TMH_HIP(hipStreamWaitEvent(h->stream, h->join_ev[i], 0));
  h->join_n = 0;
  return h->stream;
}

// The stream of an entry point: the caller's, or the handle's (joins first).
inline hipStream_t hpick(tmh_stats* h, void* stream) {
  return stream ? (hipStream_t)stream : hstream(h);
}

// the handle's stream must wait for the work queued on s so far (abi_stats.hip)
void defer_join(tmh_stats* h, hipStream_t s);

// Stream contract of the statistics entry points that take a stream
// (include/tmhip.h): on another stream than the handle's, the work runs after
// everything queued on the handle's stream (and the work joined to it), and
// the handle's stream waits for it before any later work on the handle.
// Nothing is queued on the handle's stream here: s waits for the joined
// work's events itself.
inline void cross_begin(tmh_stats* h, hipStream_t s) {
  if (s == h->stream) {
    hstream(h);
    return;
  }
  TMH_HIP(hipEventRecord(h->ev_in, h->stream));
  TMH_HIP(hipStreamWaitEvent(s, h->ev_in, 0));
  for (int i = 0; i < h->join_n; ++i)
    if (h->join_s[i] != s) TMH_HIP(hipStreamWaitEvent(s, h->join_ev[i], 0));
}
inline void cross_end(tmh_stats* h, hipStream_t s) {
  if (s == h->stream) return;
  defer_join(h, s);
}

// what the fused pass and the chain use of the statistics handle
// (abi_stats.hip) and the corrector (abi_apply.hip)
size_t os_words(const tmh_stats* h, int64_t n_sites);
void stats_reserve_sites(tmh_stats* h, int64_t n_sites);
void stats_grow_deferred(tmh_stats* h, int64_t extra);
void stats_probe(tmh_stats* h, const uint16_t* d, int64_t ns, const SiteTab& tab, hipStream_t s);
int probe_fused_cfg(const tmh_stats* h);
SiteTab blocked_tab(const uint16_t* const* dev_in_blocks, uint16_t* const* dev_out_blocks,
                    int block_shift, int64_t npx);
FixList corrector_fixlist(tmh_corrector* c, int64_t n_sites);  // the caller zeroes the count
FixList corrector_fixlist(tmh_corrector* c, int64_t n_sites, hipStream_t s);  // reset on s
void corrector_forms(tmh_corrector* c, hipStream_t s);
void check_clip(int lo, int hi, int maxv);

// feature tables of the clustering and classification tools (abi_cluster.hip)
void check_table(const void* x, int64_t n, int d);
void check_scaler(const double* center, const double* scale);
bool overlap(const void* a, size_t a_bytes, const void* b, size_t b_bytes);
// TMH_EINVAL when the table holds NaN or +-inf; cnt is the census' scratch (waits)
void require_finite(const double* dev_x, int64_t n, int d, DBuf<unsigned long long>& cnt,
                    hipStream_t s);

// label planes (abi_objects.hip): the argument checks every entry point that
// takes them shares, and the check of their labels -- the largest label of all
// planes (waits for it); TMH_EINVAL when a label is negative or above max_label
void check_planes_args(const void* planes, int64_t n_planes, int height, int width);
int32_t check_label_range(const int32_t* dev_planes, int64_t n_planes, int height, int width,
                          int32_t max_label, hipStream_t s);

// The host forms' staging of label planes, after check_planes_args, in two
// steps, because a form may have checks of its own that come between them:
// has_label_planes sets *max_label = 0 and is false when there are no planes;
// HostLabels::upload puts them on the device, rejects a negative label and
// returns *max_label, their largest.
inline bool has_label_planes(int64_t n_planes, int32_t* max_label) {
  TMH_CHECK(max_label, TMH_EINVAL, "max_label pointer is NULL");
  *max_label = 0;
  return n_planes != 0;
}
struct HostLabels {
  DBuf<int32_t> dev;
  int32_t upload(const int32_t* host_planes, int64_t n_planes, int height, int width,
                 int32_t* max_label) {
    dev.upload(host_planes, (size_t)n_planes * height * width);
    return *max_label = check_label_range(dev.p, n_planes, height, width, INT32_MAX, nullptr);
  }
};

// the host forms' staging: the table and the optional scaler on the device
struct HostTable {
  DBuf<double> x, center, scale;
  void upload(const double* host_x, int64_t n, int d, const double* host_center,
              const double* host_scale) {
    check_table(host_x, n, d);
    check_scaler(host_center, host_scale);
    x.upload(host_x, (size_t)n * d);
    if (host_center) {
      center.upload(host_center, (size_t)d);
      scale.upload(host_scale, (size_t)d);
    }
  }
};

}  // namespace tmh

#pragma GCC visibility pop
