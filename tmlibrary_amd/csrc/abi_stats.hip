// C-ABI of libtmhip.so (include/tmhip.h): the statistics handle.
#include <cstring>

#include "abi_internal.h"

namespace tmh {

// The handle's stream must wait for the work queued on s so far: recorded
// now, waited for when the handle's stream is next used (or by the next
// cross-stream call, directly).  One entry per stream.
void defer_join(tmh_stats* h, hipStream_t s) {
  int i = 0;
  while (i < h->join_n && h->join_s[i] != s) ++i;
  if (i == tmh_stats::kJoins) {  // full: join them now
    hstream(h);
    i = 0;
  }
  hipEvent_t& e = h->join_ev[i];
  if (!e) TMH_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  TMH_HIP(hipEventRecord(e, s));
  h->join_s[i] = s;
  if (i == h->join_n) ++h->join_n;
}

// words of order statistics for n sites (quantile tiles of kOsTile)
size_t os_words(const tmh_stats* h, int64_t n_sites) {
  return (size_t)n_sites * (size_t)os_tiles(h->Q) * kOsTile;
}

void stats_reserve_sites(tmh_stats* h, int64_t n_sites) {
  // growing frees buffers earlier launches may still be using
  const bool grow = (size_t)n_sites * kHiBins > h->hist_hi.n || (size_t)n_sites > h->zeros.n ||
                    ((h->flags & 2u) && (size_t)n_sites * kBins > h->site_hist.n) ||
                    (!(h->flags & TMH_STATS_DEFERRED_PCT) && os_words(h, n_sites) > h->vlh.n);
  if (grow) {
    TMH_HIP(hipStreamSynchronize(hstream(h)));
    TMH_HIP(hipStreamSynchronize(h->side));
  }
  // per-site slabs: hist_hi stays all-zero between launches (the kernel
  // resets what it touched), so it is zeroed only when (re)allocated.
  if ((size_t)n_sites * kHiBins > h->hist_hi.n) h->hist_hi.alloc((size_t)n_sites * kHiBins, true);
  h->zeros.ensure((size_t)n_sites);
  if (h->flags & 2u) h->site_hist.ensure((size_t)n_sites * kBins);
  if (!(h->flags & TMH_STATS_DEFERRED_PCT)) {
    h->vlh.ensure(os_words(h, n_sites));
  }
}

// Deferred mode keeps every site's order statistics: room for n_deferred +
// extra sites, growing geometrically; the tiles' stride is the capacity, so a
// growth re-lays the stored sites out (one 2-D copy: a row per tile).
void stats_grow_deferred(tmh_stats* h, int64_t extra) {
  const int64_t need = h->n_deferred + extra;
  if (need <= h->vlh_cap) {
    h->vlh_ld = h->vlh_cap;
    return;
  }
  const int64_t cap = std::max(need, 2 * h->vlh_cap);
  DBuf<uint32_t> nb;
  nb.alloc(os_words(h, cap));
  if (h->n_deferred) {
    const size_t row = (size_t)kOsTile * 4;
    TMH_HIP(hipMemcpy2DAsync(nb.p, (size_t)cap * row, h->vlh.p, (size_t)h->vlh_cap * row,
                             (size_t)h->n_deferred * row, (size_t)os_tiles(h->Q),
                             hipMemcpyDeviceToDevice, hstream(h)));
  }
  TMH_HIP(hipStreamSynchronize(hstream(h)));
  TMH_HIP(hipStreamSynchronize(h->side));
  std::swap(h->vlh.p, nb.p);
  std::swap(h->vlh.n, nb.n);
  h->vlh_cap = cap;
  h->vlh_ld = cap;
}

// The job's site probe, once per job (first call after a reset): one small
// kernel on s, its three counts copied to pinned memory, and the host waits
// for them -- a wait for the probe itself plus whatever s had queued before
// it.  Nothing is probed when every automatic choice is forced off.
void stats_probe(tmh_stats* h, const uint16_t* d, int64_t ns, const SiteTab& tab, hipStream_t s) {
  if (h->probed || (ns <= 0 && !h->probe_queued)) return;
  if (!h->probe_queued) {
    launch_site_probe(d, h->npx, ns, h->probe.p, s, tab);
    TMH_HIP(hipMemcpyAsync(h->probe_host, h->probe.p, 3 * sizeof(unsigned int),
                           hipMemcpyDeviceToHost, s));
    TMH_HIP(hipEventRecord(h->ev_probe, s));
  }
  TMH_HIP(hipEventSynchronize(h->ev_probe));
  for (int i = 0; i < 3; ++i) h->probe_cnt[i] = h->probe_host[i];
  h->probed = true;
  h->probe_queued = false;
}

// The probe queued ahead of the job's Welford launch (tmh_stats_probe_device):
// stats_probe then only waits for it.
static void stats_probe_queue(tmh_stats* h, const uint16_t* d, int64_t ns, const SiteTab& tab,
                              hipStream_t s) {
  if (h->probed || h->probe_queued || ns <= 0) return;
  launch_site_probe(d, h->npx, ns, h->probe.p, s, tab);
  TMH_HIP(hipMemcpyAsync(h->probe_host, h->probe.p, 3 * sizeof(unsigned int),
                         hipMemcpyDeviceToHost, s));
  TMH_HIP(hipEventRecord(h->ev_probe, s));
  h->probe_queued = true;
}

// The automatic choices from the probe (a job not probed: standard).
static bool probe_bright(const tmh_stats* h) {
  return h->probed && (double)h->probe_cnt[1] >= kBrightFrac * (double)h->probe_cnt[0];
}
int probe_fused_cfg(const tmh_stats* h) {
  if (h->fused_cfg != kFusedAuto) return h->fused_cfg;
  if (!h->probed) return kFusedNarrow;
  const double g = (double)h->probe_cnt[0];
  if ((double)h->probe_cnt[2] >= kXWideFrac * g) return kFusedNoHist;
  if ((double)h->probe_cnt[1] >= kWideFrac * g) return kFusedWide;
  return kFusedNarrow;
}

static void stats_update_dev(tmh_stats* h, const uint16_t* d, int64_t ns, int log_transform,
                             hipStream_t s) {
  if (ns <= 0) return;
  if ((size_t)ns > h->rn.n) {
    TMH_HIP(hipStreamSynchronize(s));
    h->rn.alloc((size_t)ns);
  }
  // Both passes only read the sites: run the histogram/percentile pass on a
  // side stream concurrently with the Welford pass (fork/join by events).
  const bool serial = (h->flags & TMH_STATS_SERIAL) != 0;
  hipStream_t hs = serial ? s : h->side;
  const int64_t chunk = 4096;
  stats_reserve_sites(h, std::min(chunk, ns));  // (re)allocate before forking
  if (h->flags & TMH_STATS_DEFERRED_PCT) stats_grow_deferred(h, ns);
  // the bright Welford form needs a three-part split (>= 96 sites): only then
  // is the probe worth its host wait
  const bool vec = (h->npx & 7) == 0 && (reinterpret_cast<uintptr_t>(d) & 15) == 0;
  if (vec && log_transform && h->wf_parts == 0 && ns >= 96) stats_probe(h, d, ns, SiteTab{}, s);
  if (!serial) {
    TMH_HIP(hipEventRecord(h->ev_fork, s));
    TMH_HIP(hipStreamWaitEvent(hs, h->ev_fork, 0));
  }
  launch_welford(d, h->npx, ns, h->n, h->rn.p, h->mean.p, h->m2.p, h->lut_log.p,
                 log_transform, h->wf_part.p, h->wf_part.n, h->wf_parts, nullptr,
                 probe_bright(h) ? 1 : 0, s);
  // order statistics, in chunks so the per-site slabs stay bounded
  for (int64_t c0 = 0; c0 < ns; c0 += chunk) {
    const int64_t nc = std::min(chunk, ns - c0);
    const bool deferred = (h->flags & TMH_STATS_DEFERRED_PCT) != 0;
    uint32_t* vlh = h->vlh.p + (deferred ? (size_t)h->n_deferred * kOsTile : 0);
    const int64_t ld = deferred ? h->vlh_cap : nc;
    launch_hist_scatter(d + c0 * h->npx, h->npx, nc, h->hist_hi.p, h->qp, vlh, ld, h->pooled.p,
                        h->zeros.p, (h->flags & 2u) ? h->site_hist.p : nullptr, hs);
    if (deferred)
      h->n_deferred += nc;
    else
      launch_pct_accumulate(vlh, nc, ld, h->Q, h->gamma.p, h->acc.p, hs);
    h->vlh_ld = ld;
    h->last_batch = nc;
  }
  if (!serial) {
    TMH_HIP(hipEventRecord(h->ev_join, hs));
    TMH_HIP(hipStreamWaitEvent(s, h->ev_join, 0));
  }
  h->n += ns;
}

static void stats_welford_dev(tmh_stats* h, const uint16_t* dev_sites, int64_t n_sites,
                              int log_transform, void* stream, const SiteTab& tab) {
  hipStream_t s = hpick(h, stream);
  cross_begin(h, s);
  if ((size_t)n_sites > h->rn.n) {
    TMH_HIP(hipStreamSynchronize(s));
    h->rn.alloc((size_t)n_sites);
  }
  // the probe serves the fused pass's configuration and the Welford form
  const bool vec = tab.in || ((h->npx & 7) == 0 && (reinterpret_cast<uintptr_t>(dev_sites) & 15) == 0);
  if (vec && (h->fused_cfg == kFusedAuto || (log_transform && h->wf_parts == 0)))
    stats_probe(h, dev_sites, n_sites, tab, s);
  launch_welford(dev_sites, h->npx, n_sites, h->n, h->rn.p, h->mean.p, h->m2.p, h->lut_log.p,
                 log_transform, h->wf_part.p, h->wf_part.n, h->wf_parts, h->wide.p,
                 probe_bright(h) ? 1 : 0, s, tab);
  if ((h->npx & 7) == 0) h->wide_sites += n_sites;
  h->n += n_sites;
  h->pending += n_sites;
  cross_end(h, s);
}

// a blocked site layout's table (include/tmhip.h): checked as far as the host can
SiteTab blocked_tab(const uint16_t* const* dev_in_blocks, uint16_t* const* dev_out_blocks,
                    int block_shift, int64_t npx) {
  TMH_CHECK(dev_in_blocks, TMH_EINVAL, "block table is NULL");
  TMH_CHECK(block_shift >= 2 && block_shift <= 24, TMH_EINVAL, "block_shift must be 2..24");
  TMH_CHECK((npx & 7) == 0, TMH_EINVAL,
            "blocked site layouts need height * width divisible by 8 (16-byte pixel groups)");
  SiteTab t;
  t.in = dev_in_blocks;
  t.out = dev_out_blocks;
  t.shift = block_shift;
  return t;
}

static void stats_pct_sum_device(tmh_stats* h) {
  if ((h->flags & TMH_STATS_DEFERRED_PCT) && !h->pct_sum_external) {
    TMH_HIP(hipMemsetAsync(h->acc.p, 0, (size_t)h->Q * 8, hstream(h)));
    launch_pct_accumulate(h->vlh.p, h->n_deferred, h->vlh_cap, h->Q, h->gamma.p, h->acc.p,
                          hstream(h));
  }
}

}  // namespace tmh

extern "C" {

int tmh_stats_create(int height, int width, int n_quantiles, const int64_t* q_lo,
                     const int64_t* q_hi, const double* q_gamma, const double* lut_log10,
                     int batch_capacity, unsigned flags, tmh_stats** out) {
  return guard([&] {
    TMH_CHECK(out, TMH_EINVAL, "out is NULL");
    TMH_CHECK(height > 0 && width > 0, TMH_EINVAL, "image dimensions must be positive");
    const int64_t npx = (int64_t)height * width;
    TMH_CHECK(npx < (int64_t(1) << 31), TMH_EINVAL, "images must have fewer than 2^31 pixels");
    TMH_CHECK(n_quantiles > 0 && q_lo && q_hi && q_gamma && lut_log10, TMH_EINVAL,
              "quantile tables and LUT are required");
    auto* h = new tmh_stats();
    try {
      TMH_HIP(hipGetDevice(&h->device));
      h->H = height;
      h->W = width;
      h->npx = npx;
      h->Q = n_quantiles;
      h->scale = (npx > 1) ? (double)(n_quantiles - 1) / (double)(npx - 1) : 0.0;
      h->flags = flags;
      h->batch_cap = std::min(4096, batch_capacity > 0 ? batch_capacity : 1);
      TMH_HIP(hipStreamCreateWithFlags(&h->own_stream, hipStreamNonBlocking));
      TMH_HIP(hipStreamCreateWithFlags(&h->side, hipStreamNonBlocking));

      TMH_HIP(hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming));
      TMH_HIP(hipEventCreateWithFlags(&h->ev_join, hipEventDisableTiming));
      TMH_HIP(hipEventCreateWithFlags(&h->ev_in, hipEventDisableTiming));
      TMH_HIP(hipEventCreateWithFlags(&h->ev_out, hipEventDisableTiming));
      h->stream = h->own_stream;
      h->mean.alloc(npx, true);
      h->m2.alloc(npx, true);
      h->wf_part.alloc((size_t)8 * npx);
      h->wide.alloc(2, true);  // groups with a value >= 4,096 / >= 16,384
      h->probe.alloc(3);
      TMH_HIP(hipHostMalloc((void**)&h->probe_host, 4 * sizeof(unsigned int), hipHostMallocDefault));
      TMH_HIP(hipEventCreateWithFlags(&h->ev_probe, hipEventDisableTiming));
      h->acc.alloc(n_quantiles, true);
      h->pooled.alloc(kBins, true);
      h->lut_log.alloc(kBins);
      h->gamma.alloc(n_quantiles);
      h->q_lo.alloc(n_quantiles);
      h->q_hi.alloc(n_quantiles);
      std::vector<int32_t> lo(n_quantiles), hi(n_quantiles);
      for (int i = 0; i < n_quantiles; ++i) {
        TMH_CHECK(q_lo[i] >= 0 && q_lo[i] < npx && q_hi[i] >= q_lo[i] && q_hi[i] < npx, TMH_EINVAL,
                  "quantile positions out of range");
        TMH_CHECK(i == 0 || (q_lo[i] >= q_lo[i - 1] && q_hi[i] >= q_hi[i - 1]), TMH_EINVAL,
                  "quantile positions must be non-decreasing");
        lo[i] = (int32_t)q_lo[i];
        hi[i] = (int32_t)q_hi[i];
      }
      TMH_HIP(hipMemcpy(h->q_lo.p, lo.data(), lo.size() * 4, hipMemcpyHostToDevice));
      TMH_HIP(hipMemcpy(h->q_hi.p, hi.data(), hi.size() * 4, hipMemcpyHostToDevice));
      TMH_HIP(hipMemcpy(h->gamma.p, q_gamma, (size_t)n_quantiles * 8, hipMemcpyHostToDevice));
      TMH_HIP(hipMemcpy(h->lut_log.p, lut_log10, (size_t)kBins * 8, hipMemcpyHostToDevice));
      h->pooled_parts.alloc((size_t)kPooledParts * kBins, true);
      h->qp.lo = h->q_lo.p;
      h->qp.hi = h->q_hi.p;
      h->qp.Q = n_quantiles;
      h->qp.scale = h->scale;
      h->qp.last = (int32_t)(npx - 1);
      h->qp.hi_next = 1;
      for (int i = 0; i < n_quantiles; ++i)
        if (hi[i] != std::min<int32_t>(lo[i] + 1, (int32_t)(npx - 1))) h->qp.hi_next = 0;
    } catch (...) {
      tmh_stats_destroy(h);
      throw;
    }
    *out = h;
  });
}

void tmh_stats_destroy(tmh_stats* h) {
  if (!h) return;
  for (int i = 0; i < h->join_n; ++i) (void)hipEventSynchronize(h->join_ev[i]);
  if (h->own_stream) (void)hipStreamSynchronize(h->own_stream);
  if (h->stream && h->stream != h->own_stream) (void)hipStreamSynchronize(h->stream);
  hipStream_t s = h->own_stream, side = h->side, tail = h->tail;
  if (side) (void)hipStreamSynchronize(side);
  if (tail) (void)hipStreamSynchronize(tail);
  if (h->ev_fork) (void)hipEventDestroy(h->ev_fork);
  if (h->ev_join) (void)hipEventDestroy(h->ev_join);
  if (h->ev_in) (void)hipEventDestroy(h->ev_in);
  if (h->ev_out) (void)hipEventDestroy(h->ev_out);
  if (h->ev_probe) (void)hipEventDestroy(h->ev_probe);
  for (hipEvent_t e : h->join_ev)
    if (e) (void)hipEventDestroy(e);
  if (h->probe_host) (void)hipHostFree(h->probe_host);
  delete h;
  if (s) (void)hipStreamDestroy(s);
  if (side) (void)hipStreamDestroy(side);
  if (tail) (void)hipStreamDestroy(tail);
}

int tmh_stats_set_stream(tmh_stats* h, void* stream) {
  return guard([&] {
    TMH_CHECK(h, TMH_EINVAL, "handle is NULL");
    h->stream = stream ? (hipStream_t)stream : h->own_stream;
  });
}

int tmh_stats_set_option(tmh_stats* h, int option, int value) {
  return guard([&] {
    TMH_CHECK(h, TMH_EINVAL, "handle is NULL");
    switch (option) {
      case TMH_OPT_FUSED_CONFIG:
        TMH_CHECK(value < 0 || value > 4 || value == kFusedNarrow, TMH_EINVAL,
                  "fused configuration retired (measured slower): 3, 5 and 100 remain");
        TMH_CHECK(value == kFusedAuto || value == kFusedNarrow || value == kFusedWide ||
                      value == kFusedNoHist,
                  TMH_EINVAL, "fused configuration out of range");
        h->fused_cfg = value;
        break;
      case TMH_OPT_WELFORD_PARTS:
        TMH_CHECK(value >= 0 && value <= 4, TMH_EINVAL, "Welford parts must be 0..4");
        h->wf_parts = value;
        break;
      default:
        if (!h->host.set(option, value)) throw Error{TMH_EINVAL, "unknown option"};
    }
  });
}

int tmh_stats_reset(tmh_stats* h) {
  return guard([&] {
    TMH_CHECK(h, TMH_EINVAL, "handle is NULL");
    if (h->hist_dirty) {  // an interrupted fused launch: restore the zero-maintained slabs
      TMH_HIP(hipDeviceSynchronize());  // it may have been queued on any stream
      if (h->hist_full.n)
        TMH_HIP(hipMemsetAsync(h->hist_full.p, 0, h->hist_full.n * 4, hstream(h)));
      if (h->hist_rmask.n)
        TMH_HIP(hipMemsetAsync(h->hist_rmask.p, 0, h->hist_rmask.n * 8, hstream(h)));
      TMH_HIP(hipMemsetAsync(h->pooled_parts.p, 0, h->pooled_parts.n * 8, hstream(h)));
      h->hist_dirty = false;
    }
    ZeroList z;  // one launch for the job's fresh state
    z.add(h->mean.p, h->npx);
    z.add(h->m2.p, h->npx);
    z.add(h->acc.p, h->Q);
    z.add(h->pooled.p, kBins);
    z.add(h->wide.p, 2);
    launch_zero_u64(z, hstream(h));
    h->wide_sites = 0;
    h->n = 0;
    h->n_deferred = 0;
    h->last_batch = 0;
    h->pending = 0;
    h->pct_sum_external = false;
    if (h->probe_queued) TMH_HIP(hipEventSynchronize(h->ev_probe));  // its buffers are reused
    h->probed = false;  // the next job probes its own sites
    h->probe_queued = false;
  });
}

int tmh_stats_probe_device(tmh_stats* h, const uint16_t* dev_sites, int64_t n_sites,
                           void* stream) {
  return guard([&] {
    TMH_CHECK(h && (dev_sites || n_sites == 0) && n_sites >= 0, TMH_EINVAL, "bad arguments");
    if ((h->npx & 7) || (reinterpret_cast<uintptr_t>(dev_sites) & 15)) return;  // no vector path
    // ordered after stream's work only (include/tmhip.h): the counts go to the host
    stats_probe_queue(h, dev_sites, n_sites, SiteTab{}, hpick(h, stream));
  });
}

int tmh_stats_probe_blocks_device(tmh_stats* h, const uint16_t* const* dev_blocks, int block_shift,
                                  int64_t n_sites, void* stream) {
  return guard([&] {
    TMH_CHECK(h && n_sites >= 0, TMH_EINVAL, "bad arguments");
    const SiteTab tab = blocked_tab(dev_blocks, nullptr, block_shift, h->npx);
    stats_probe_queue(h, nullptr, n_sites, tab, hpick(h, stream));
  });
}

int tmh_stats_update_welford_device(tmh_stats* h, const uint16_t* dev_sites, int64_t n_sites,
                                    int log_transform, void* stream) {
  return guard([&] {
    TMH_CHECK(h && (dev_sites || n_sites == 0) && n_sites >= 0, TMH_EINVAL, "bad arguments");
    stats_welford_dev(h, dev_sites, n_sites, log_transform, stream, SiteTab{});
  });
}

int tmh_stats_update_welford_blocks_device(tmh_stats* h, const uint16_t* const* dev_blocks,
                                           int block_shift, int64_t n_sites, int log_transform,
                                           void* stream) {
  return guard([&] {
    TMH_CHECK(h && n_sites >= 0, TMH_EINVAL, "bad arguments");
    if (n_sites == 0) return;
    stats_welford_dev(h, nullptr, n_sites, log_transform, stream,
                      blocked_tab(dev_blocks, nullptr, block_shift, h->npx));
  });
}

int tmh_stats_update_device(tmh_stats* h, const uint16_t* dev_sites, int64_t n_sites,
                            int log_transform, void* stream) {
  return guard([&] {
    TMH_CHECK(h && (dev_sites || n_sites == 0) && n_sites >= 0, TMH_EINVAL, "bad arguments");
    const hipStream_t s = hpick(h, stream);
    cross_begin(h, s);
    stats_update_dev(h, dev_sites, n_sites, log_transform, s);
    cross_end(h, s);
  });
}

int tmh_stats_zero_counts(tmh_stats* h, int64_t* host_out, int64_t n, void* stream) {
  return guard([&] {
    TMH_CHECK(h && (host_out || n == 0) && n >= 0, TMH_EINVAL, "bad arguments");
    TMH_CHECK(n <= h->last_batch && (size_t)n <= h->zeros.n, TMH_EINVAL,
              "more sites than the last update held");
    if (n == 0) return;
    hipStream_t s = hpick(h, stream);
    cross_begin(h, s);
    TMH_HIP(hipMemcpyAsync(host_out, h->zeros.p, (size_t)n * 8, hipMemcpyDeviceToHost, s));
    cross_end(h, s);  // a later update (on any stream) writes h->zeros after this copy
  });
}

int tmh_stats_update(tmh_stats* h, const uint16_t* host_sites, int64_t n_sites, int log_transform,
                     int64_t* zero_counts_out) {
  return guard([&] {
    TMH_CHECK(h && (host_sites || n_sites == 0) && n_sites >= 0, TMH_EINVAL, "bad arguments");
    if (n_sites == 0) return;
    HostPipe& p = h->pipe;
    const int64_t per = h->batch_cap;
    const size_t slot_px = (size_t)per * h->npx;
    if (2 * slot_px > h->stage.n) {
      TMH_HIP(hipStreamSynchronize(hstream(h)));
      h->stage.ensure(2 * slot_px);
    }
    p.init();
    // retire chunk k-2 of this slot: its H2D, kernels and zero-count copy
    auto retire = [&](int slot) {
      if (!p.busy[slot]) return;
      TMH_HIP(hipEventSynchronize(p.ev_done[slot]));
      if (zero_counts_out)
        std::memcpy(zero_counts_out + p.s0[slot], p.out[slot].p, (size_t)p.ns[slot] * 8);
      p.busy[slot] = false;
    };
    int64_t k = 0;
    try {
      for (int64_t s0 = 0; s0 < n_sites; s0 += per, ++k) {
        const int slot = (int)(k & 1);
        const int64_t ns = std::min<int64_t>(per, n_sites - s0);
        const size_t bytes = (size_t)ns * h->npx * 2;
        retire(slot);
        p.out[slot].ensure((size_t)per * 8);
        uint16_t* dev = h->stage.p + (size_t)slot * slot_px;
        TMH_HIP(hipMemcpyAsync(dev, host_sites + s0 * h->npx, bytes, hipMemcpyHostToDevice, p.h2d));
        TMH_HIP(hipEventRecord(p.ev_in[slot], p.h2d));
        TMH_HIP(hipStreamWaitEvent(hstream(h), p.ev_in[slot], 0));
        stats_update_dev(h, dev, ns, log_transform, hstream(h));
        if (zero_counts_out)
          TMH_HIP(hipMemcpyAsync(p.out[slot].p, h->zeros.p, (size_t)ns * 8, hipMemcpyDeviceToHost,
                                 hstream(h)));
        TMH_HIP(hipEventRecord(p.ev_done[slot], hstream(h)));
        p.busy[slot] = true;
        p.s0[slot] = s0;
        p.ns[slot] = ns;
      }
      retire((int)(k & 1));
      retire((int)((k + 1) & 1));
    } catch (...) {
      p.abandon(hstream(h));
      throw;
    }
  });
}

int tmh_stats_finalize(tmh_stats* h, int64_t* n, double* mean, double* std, double* pct_sum,
                       uint64_t* hist) {
  return guard([&] {
    TMH_CHECK(h, TMH_EINVAL, "handle is NULL");
    if (n) *n = h->n;
    if (mean || std) {
      h->tmp_std.ensure(h->npx);
      launch_finalize(h->mean.p, h->m2.p, h->n, h->npx, nullptr, h->tmp_std.p, hstream(h));
      if (mean)
        TMH_HIP(hipMemcpyAsync(mean, h->mean.p, h->npx * 8, hipMemcpyDeviceToHost, hstream(h)));
      if (std)
        TMH_HIP(hipMemcpyAsync(std, h->tmp_std.p, h->npx * 8, hipMemcpyDeviceToHost, hstream(h)));
    }
    if (pct_sum) {
      stats_pct_sum_device(h);
      TMH_HIP(hipMemcpyAsync(pct_sum, h->acc.p, (size_t)h->Q * 8, hipMemcpyDeviceToHost, hstream(h)));
    }
    if (hist)
      TMH_HIP(hipMemcpyAsync(hist, h->pooled.p, (size_t)kBins * 8, hipMemcpyDeviceToHost, hstream(h)));
    TMH_HIP(hipStreamSynchronize(hstream(h)));
  });
}

int tmh_stats_finalize_device(tmh_stats* h, double* dev_mean, double* dev_std, void* stream) {
  return guard([&] {
    TMH_CHECK(h, TMH_EINVAL, "handle is NULL");
    const hipStream_t s = hpick(h, stream);
    cross_begin(h, s);
    launch_finalize(h->mean.p, h->m2.p, h->n, h->npx, dev_mean, dev_std, s);
    cross_end(h, s);
  });
}

int tmh_stats_variance(tmh_stats* h, double* host_var) {
  return guard([&] {
    TMH_CHECK(h && host_var, TMH_EINVAL, "bad arguments");
    h->tmp_std.ensure(h->npx);
    launch_variance(h->m2.p, h->n, h->npx, h->tmp_std.p, hstream(h));
    TMH_HIP(hipMemcpyAsync(host_var, h->tmp_std.p, h->npx * 8, hipMemcpyDeviceToHost, hstream(h)));
    TMH_HIP(hipStreamSynchronize(hstream(h)));
  });
}

int tmh_stats_job_choice(tmh_stats* h, uint32_t* probe_counts, int* welford_bright,
                         int* fused_cfg) {
  return guard([&] {
    TMH_CHECK(h, TMH_EINVAL, "handle is NULL");
    if (probe_counts)
      for (int i = 0; i < 3; ++i) probe_counts[i] = h->probed ? h->probe_cnt[i] : 0u;
    if (welford_bright) *welford_bright = h->probed ? (probe_bright(h) ? 1 : 0) : -1;
    if (fused_cfg) {
      const int c = probe_fused_cfg(h);
      *fused_cfg = c == kFusedNoHist ? TMH_FUSED_NO_HIST : c;
    }
  });
}

int tmh_stats_wide_groups(tmh_stats* h, uint64_t* groups_out, int64_t* sites_out) {
  return guard([&] {
    TMH_CHECK(h && groups_out, TMH_EINVAL, "bad arguments");
    unsigned long long w = 0;
    TMH_HIP(hipMemcpyAsync(&w, h->wide.p, 8, hipMemcpyDeviceToHost, hstream(h)));
    TMH_HIP(hipStreamSynchronize(hstream(h)));
    *groups_out = w;
    if (sites_out) *sites_out = h->wide_sites;
  });
}

int tmh_stats_get_hist_device(tmh_stats* h, uint64_t* dev_hist, void* stream) {
  return guard([&] {
    TMH_CHECK(h && dev_hist, TMH_EINVAL, "bad arguments");
    const hipStream_t s = hpick(h, stream);
    cross_begin(h, s);
    TMH_HIP(hipMemcpyAsync(dev_hist, h->pooled.p, (size_t)kBins * 8, hipMemcpyDeviceToDevice, s));
    cross_end(h, s);
  });
}

int tmh_stats_set_hist_device(tmh_stats* h, const uint64_t* dev_hist, void* stream) {
  return guard([&] {
    TMH_CHECK(h && dev_hist, TMH_EINVAL, "bad arguments");
    const hipStream_t s = hpick(h, stream);
    cross_begin(h, s);
    TMH_HIP(hipMemcpyAsync(h->pooled.p, dev_hist, (size_t)kBins * 8, hipMemcpyDeviceToDevice, s));
    cross_end(h, s);
  });
}

int tmh_stats_site_histogram(tmh_stats* h, int64_t site, uint32_t* host_hist) {
  return guard([&] {
    TMH_CHECK(h && host_hist, TMH_EINVAL, "bad arguments");
    TMH_CHECK(h->flags & 2u, TMH_ESTATE, "handle was created without TMH_STATS_KEEP_SITE_HIST (2)");
    TMH_CHECK(site >= 0 && site < h->last_batch, TMH_EINVAL, "site outside the last batch");
    TMH_HIP(hipMemcpyAsync(host_hist, h->site_hist.p + (size_t)site * kBins, (size_t)kBins * 4,
                           hipMemcpyDeviceToHost, hstream(h)));
    TMH_HIP(hipStreamSynchronize(hstream(h)));
  });
}

int tmh_stats_site_order_stats(tmh_stats* h, int64_t site, uint16_t* host_vlo, uint16_t* host_vhi) {
  return guard([&] {
    TMH_CHECK(h && host_vlo && host_vhi, TMH_EINVAL, "bad arguments");
    const bool deferred = h->flags & TMH_STATS_DEFERRED_PCT;
    const int64_t avail = deferred ? h->n_deferred : h->last_batch;
    TMH_CHECK(site >= 0 && site < avail, TMH_EINVAL, "site not available");
    // one site's column of every quantile tile
    const size_t row = (size_t)kOsTile * 4;
    std::vector<uint32_t> w((size_t)os_tiles(h->Q) * kOsTile);
    TMH_HIP(hipMemcpy2DAsync(w.data(), row, h->vlh.p + (size_t)site * kOsTile,
                             (size_t)h->vlh_ld * row, row, (size_t)os_tiles(h->Q),
                             hipMemcpyDeviceToHost, hstream(h)));
    TMH_HIP(hipStreamSynchronize(hstream(h)));
    for (int64_t q = 0; q < h->Q; ++q) {
      host_vlo[q] = (uint16_t)(w[q] & 0xFFFFu);
      host_vhi[q] = (uint16_t)(w[q] >> 16);
    }
    TMH_HIP(hipStreamSynchronize(hstream(h)));
  });
}

int tmh_stats_get_n(tmh_stats* h, int64_t* n) {
  return guard([&] {
    TMH_CHECK(h && n, TMH_EINVAL, "bad arguments");
    *n = h->n;
  });
}

int tmh_stats_set_n(tmh_stats* h, int64_t n) {
  return guard([&] {
    TMH_CHECK(h && n >= 0, TMH_EINVAL, "bad arguments");
    h->n = n;
  });
}

int tmh_stats_merge_stage1(tmh_stats* h, double* dev_nmean, void* stream) {
  return guard([&] {
    TMH_CHECK(h && dev_nmean, TMH_EINVAL, "bad arguments");
    const hipStream_t s = hpick(h, stream);
    cross_begin(h, s);
    launch_merge1(h->mean.p, h->n, h->npx, dev_nmean, s);
    cross_end(h, s);
  });
}

int tmh_stats_merge_stage2(tmh_stats* h, const double* dev_sum_nmean, int64_t n_total,
                           double* dev_m2c, void* stream) {
  return guard([&] {
    TMH_CHECK(h && dev_sum_nmean && dev_m2c && n_total > 0, TMH_EINVAL, "bad arguments");
    const hipStream_t s = hpick(h, stream);
    cross_begin(h, s);
    launch_merge2(h->mean.p, h->m2.p, h->n, dev_sum_nmean, n_total, h->npx, dev_m2c, s);
    cross_end(h, s);
  });
}

int tmh_stats_merge_stage3(tmh_stats* h, int64_t n_total, const double* dev_sum_m2c, void* stream) {
  return guard([&] {
    TMH_CHECK(h && dev_sum_m2c && n_total >= 0, TMH_EINVAL, "bad arguments");
    const hipStream_t s = hpick(h, stream);
    cross_begin(h, s);
    launch_copy_f64(dev_sum_m2c, h->m2.p, h->npx, s);
    cross_end(h, s);
    h->n = n_total;
  });
}

int tmh_stats_pct_accumulate(tmh_stats* h, double* dev_acc, void* stream) {
  return guard([&] {
    TMH_CHECK(h && dev_acc, TMH_EINVAL, "bad arguments");
    TMH_CHECK(h->flags & TMH_STATS_DEFERRED_PCT, TMH_ESTATE,
              "percentile chain needs a TMH_STATS_DEFERRED_PCT handle");
    const hipStream_t s = hpick(h, stream);
    cross_begin(h, s);
    launch_pct_accumulate(h->vlh.p, h->n_deferred, h->vlh_cap, h->Q, h->gamma.p, dev_acc, s);
    cross_end(h, s);
  });
}

int tmh_stats_pct_accumulate_range(tmh_stats* h, double* dev_acc_range, int q_begin, int q_count,
                                   void* stream) {
  return guard([&] {
    TMH_CHECK(h && dev_acc_range, TMH_EINVAL, "bad arguments");
    TMH_CHECK(h->flags & TMH_STATS_DEFERRED_PCT, TMH_ESTATE,
              "percentile chain needs a TMH_STATS_DEFERRED_PCT handle");
    TMH_CHECK(q_begin >= 0 && q_count >= 0 && (int64_t)q_begin + q_count <= h->Q, TMH_EINVAL,
              "quantile range out of bounds");
    const hipStream_t s = hpick(h, stream);
    cross_begin(h, s);
    launch_pct_accumulate_range(h->vlh.p, h->n_deferred, h->vlh_cap, q_begin, q_count, h->gamma.p,
                                dev_acc_range, s);
    cross_end(h, s);
  });
}

int tmh_stats_set_pct_sum(tmh_stats* h, const double* dev_acc, void* stream) {
  return guard([&] {
    TMH_CHECK(h && dev_acc, TMH_EINVAL, "bad arguments");
    const hipStream_t s = hpick(h, stream);
    cross_begin(h, s);
    launch_copy_f64(dev_acc, h->acc.p, h->Q, s);
    cross_end(h, s);
    h->pct_sum_external = true;
  });
}

int tmh_stats_get_pct_sum_device(tmh_stats* h, double* dev_acc, void* stream) {
  return guard([&] {
    TMH_CHECK(h && dev_acc, TMH_EINVAL, "bad arguments");
    hipStream_t s = hpick(h, stream);
    const bool cross = s != h->stream;
    cross_begin(h, s);  // after the handle's queued work, and the handle waits for the copy
    if ((h->flags & TMH_STATS_DEFERRED_PCT) && !h->pct_sum_external) {
      TMH_HIP(hipMemsetAsync(dev_acc, 0, (size_t)h->Q * 8, s));
      launch_pct_accumulate(h->vlh.p, h->n_deferred, h->vlh_cap, h->Q, h->gamma.p, dev_acc, s);
    } else {
      TMH_HIP(hipMemcpyAsync(dev_acc, h->acc.p, (size_t)h->Q * 8, hipMemcpyDeviceToDevice, s));
    }
    if (cross) defer_join(h, s);
  });
}

}  // extern "C"
