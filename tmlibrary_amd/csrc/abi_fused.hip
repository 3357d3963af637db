// C-ABI of libtmhip.so (include/tmhip.h): the fused correct + histogram pass.
#include "abi_internal.h"

namespace tmh {

// One job's fused pass (correct + per-site histograms, then the histogram
// tail), in steps so several jobs can share the launches in between
// (correct_hist_multi): fused_prepare -> resets, launch, fixups -> fused_post
// -> the tail (fused_tail, or every job's at once and fused_tail_end).
struct FusedPass {
  tmh_corrector* c;
  tmh_stats* h;
  const uint16_t* in;
  uint16_t* out;
  int64_t n;
  SiteTab tab;
  hipStream_t s;
  bool cross;
  int clip_lo, clip_hi;
  int cfg;
  RareList rl;
  FixList fl;
  uint32_t* vlh;
  int64_t ld;
  uint32_t* sh;
};

// the fused pass floors zero pixels at 10**zero_log10 in f32 and reads 8-pixel
// groups: false = the two-pass path for odd shapes
static bool fused_vec(const tmh_corrector* c, const tmh_stats* h, const uint16_t* dev_in,
                      const uint16_t* dev_out, const SiteTab& tab) {
  const bool zl_ok = !c->log_transform || (c->zero_log10 >= -37.0 && c->zero_log10 <= 0.0);
  const bool vec = zl_ok && (h->npx & 7) == 0 &&
                   (tab.in || ((reinterpret_cast<uintptr_t>(dev_in) & 15) == 0 &&
                               (reinterpret_cast<uintptr_t>(dev_out) & 15) == 0));
  TMH_CHECK(vec || !tab.in, TMH_EINVAL,
            "a blocked site layout needs the fused pass (zero_log10 in [-37, 0])");
  return vec;
}

static void fused_check(const tmh_corrector* c, const tmh_stats* h, int64_t n_sites) {
  TMH_CHECK(c->npx == h->npx, TMH_EINVAL, "corrector and statistics image sizes differ");
  TMH_CHECK(n_sites <= h->pending, TMH_ESTATE,
            "more sites than were passed to tmh_stats_update_welford_device");
}

// Stream contract (include/tmhip.h): the job's launches run on s, after
// everything already queued on the statistics handle's stream (and after the
// corrector's pending tail, which still reads its round masks).
static bool fused_begin(tmh_corrector* c, tmh_stats* h, hipStream_t s) {
  const bool cross = s != h->stream;
  cross_begin(h, s);
  if (c->tail_pending) {
    TMH_HIP(hipStreamWaitEvent(s, c->ev_tail, 0));
    c->tail_pending = false;
  }
  return cross;
}

// The per-site buffers of a pass over n_sites sites and where its order
// statistics go (vlh, of a buffer with room for ld sites).  Growing frees
// memory earlier launches may still use: the streams are drained first (more:
// the caller has buffers of its own to grow after this).
static void pass_buffers(tmh_stats* h, int64_t n_sites, hipStream_t s, bool more, uint32_t*& vlh,
                         int64_t& ld) {
  const bool grow = more || (size_t)n_sites > h->zeros.n ||
                    ((h->flags & 2u) && (size_t)n_sites * kBins > h->site_hist.n) ||
                    (!(h->flags & TMH_STATS_DEFERRED_PCT) && os_words(h, n_sites) > h->vlh.n);
  if (grow) {
    TMH_HIP(hipStreamSynchronize(s));
    TMH_HIP(hipStreamSynchronize(hstream(h)));
    TMH_HIP(hipStreamSynchronize(h->side));
  }
  h->zeros.ensure((size_t)n_sites);
  if (h->flags & 2u) h->site_hist.ensure((size_t)n_sites * kBins);
  if (h->flags & TMH_STATS_DEFERRED_PCT) {
    stats_grow_deferred(h, n_sites);
    vlh = h->vlh.p + (size_t)h->n_deferred * kOsTile;
    ld = h->vlh_cap;
  } else {
    h->vlh.ensure(os_words(h, n_sites));
    vlh = h->vlh.p;
    ld = n_sites;
  }
  h->vlh_ld = ld;
}

// buffers, rare lists, fixup list and the configuration of one job's pass
// (the caller zeroes the fixup counter and the unit queues with its other jobs')
static void fused_prepare(FusedPass& p) {
  tmh_stats* h = p.h;
  const int64_t n_sites = p.n;
  hipStream_t s = p.s;
  // rare lists (RareList, common.h) for the packed configuration
  if (h->fused_cfg == kFusedAuto) stats_probe(h, p.in, n_sites, p.tab, s);
  const bool rl_on = probe_fused_cfg(h) == kFusedWide;
  const unsigned int rl_cap =
      (unsigned int)std::min<int64_t>(65536, std::max<int64_t>(1024, h->npx / 64));
  const bool more = (size_t)n_sites * kBins > h->hist_full.n || (size_t)n_sites > h->hist_rmask.n ||
                    (rl_on && ((size_t)n_sites * rl_cap > h->rare_v.n ||
                               (size_t)n_sites > h->rare_n.n));
  pass_buffers(h, n_sites, s, more, p.vlh, p.ld);
  if ((size_t)n_sites * kBins > h->hist_full.n) h->hist_full.alloc((size_t)n_sites * kBins, true);
  if ((size_t)n_sites > h->hist_rmask.n) h->hist_rmask.alloc((size_t)n_sites, true);
  p.rl = RareList{};
  if (rl_on) {
    h->rare_v.ensure((size_t)n_sites * rl_cap);
    h->rare_n.ensure((size_t)n_sites);
    TMH_HIP(hipMemsetAsync(h->rare_n.p, 0, (size_t)n_sites * sizeof(unsigned int), s));
    p.rl = RareList{h->rare_v.p, h->rare_n.p, rl_cap};
  }
  // the histogram slab and round masks are zero-maintained: the fused pass
  // fills them and k_hist_finalize resets what it read; if anything fails in
  // between, tmh_stats_reset clears them (hist_dirty)
  h->hist_dirty = true;
  p.sh = (h->flags & 2u) ? h->site_hist.p : nullptr;
  // one configuration, chosen on the host from the job's site probe (probed
  // at the Welford launch, or above for a job whose Welford pass did not)
  p.cfg = probe_fused_cfg(h);
  p.fl = corrector_fixlist(p.c, n_sites);
}

// what follows the job's fused launch and fixups up to its histogram tail:
// rare lists and the very wide configuration's histograms
static void fused_post(FusedPass& p) {
  tmh_stats* h = p.h;
  const int64_t n_sites = p.n;
  hipStream_t s = p.s;
  if (p.cfg == kFusedWide) launch_rare_count(p.rl, h->hist_full.p, n_sites, s);
  if (p.cfg == kFusedNoHist)  // the histograms from one more read of the sites
    launch_hist_site_u16(p.in, h->npx, n_sites, h->hist_full.p, h->qp, p.vlh, p.ld, h->pooled.p,
                         h->pooled_parts.p, h->zeros.p, p.sh, s, p.tab);
  // the Welford pass's diagnostic wide counts restart with the next batch
  // (the fixup launch reset them on s, before any later Welford launch on
  // the handle)
  if (h->pending - n_sites == 0) h->wide_sites = 0;
}

// The histogram tail (order statistics, percentile sums) reads only the
// handle's buffers: called on another stream than the handle's, it runs on
// the handle's tail stream (the handle's stream waits for it), so s is free
// as soon as the corrected sites are written (a caller pipelining jobs
// starts the next one's Welford pass under this one's tail).
static hipStream_t fused_tail_stream(const FusedPass& p) {
  tmh_stats* h = p.h;
  if (!p.cross) return p.s;
  if (!h->tail) {  // created on first use: every stream takes a hardware queue slot
    TMH_HIP(hipStreamCreateWithFlags(&h->tail, hipStreamNonBlocking));
  }
  TMH_HIP(hipEventRecord(h->ev_out, p.s));
  TMH_HIP(hipStreamWaitEvent(h->tail, h->ev_out, 0));
  return h->tail;
}

// the tail's percentile sums and the handle's bookkeeping; ts: the stream
// the job's order statistics were queued on
static void fused_tail_end(FusedPass& p, hipStream_t ts) {
  tmh_stats* h = p.h;
  tmh_corrector* c = p.c;
  const int64_t n_sites = p.n;
  if (!(h->flags & TMH_STATS_DEFERRED_PCT))
    launch_pct_accumulate(p.vlh, n_sites, p.ld, h->Q, h->gamma.p, h->acc.p, ts);
  h->hist_dirty = false;
  if (h->flags & TMH_STATS_DEFERRED_PCT) h->n_deferred += n_sites;
  h->last_batch = n_sites;
  h->pending -= n_sites;
  if (p.cross) {  // the handle's later work, and this corrector's next pass, after the tail
    defer_join(h, ts);
    if (!c->ev_tail) TMH_HIP(hipEventCreateWithFlags(&c->ev_tail, hipEventDisableTiming));
    TMH_HIP(hipEventRecord(c->ev_tail, ts));
    c->tail_pending = true;
  }
}

// what the histogram tail reads and writes for the job
static TailJob tail_job(const FusedPass& p) {
  tmh_stats* h = p.h;
  QPos qp = h->qp;
  qp.tstride = p.ld * kOsTile;
  return TailJob{h->hist_full.p, h->hist_rmask.p,
                 reinterpret_cast<const unsigned long long*>(p.c->queues.p + 8), qp,
                 p.vlh, h->pooled.p, h->zeros.p, p.sh, p.n};
}

// one job's histogram tail, on its handle's tail stream (or s)
static void fused_tail(FusedPass& p) {
  hipStream_t ts = fused_tail_stream(p);
  if (p.cfg != kFusedNoHist)  // (very wide: k_hist_site_u16 wrote the order statistics)
    launch_hist_finalize(tail_job(p), ts);
  fused_tail_end(p, ts);
}

// Odd shapes (fused_vec): correct and histogram in two passes
static void correct_hist_two_pass(tmh_corrector* c, tmh_stats* h, const uint16_t* dev_in,
                                  uint16_t* dev_out, int64_t n_sites, int clip_lo, int clip_hi,
                                  hipStream_t s) {
  const bool cross = fused_begin(c, h, s);
  const int64_t chunk = 4096;
  for (int64_t c0 = 0; c0 < n_sites; c0 += chunk) {
    const int64_t nc = std::min(chunk, n_sites - c0);
    const uint16_t* din = dev_in + c0 * h->npx;
    uint16_t* dout = dev_out + c0 * h->npx;
    uint32_t* vlh;
    int64_t ld;
    pass_buffers(h, nc, s, false, vlh, ld);
    stats_reserve_sites(h, nc);
    const FixList fl = corrector_fixlist(c, nc, s);
    corrector_forms(c, s);
    launch_correct_u16(din, dout, c->npx, nc, c->coef.p, c->lut.p, c->mconst.p, fl,
                       c->log_transform, clip_lo, clip_hi, s);
    launch_fix_correct(din, dout, 2, c->npx, nc, fl, c->coef64.p, c->rc.p, c->log_transform,
                       clip_lo, clip_hi, s);
    launch_hist_scatter(din, h->npx, nc, h->hist_hi.p, h->qp, vlh, ld, h->pooled.p, h->zeros.p,
                        (h->flags & 2u) ? h->site_hist.p : nullptr, s);
    if (h->flags & TMH_STATS_DEFERRED_PCT)
      h->n_deferred += nc;
    else
      launch_pct_accumulate(vlh, nc, ld, h->Q, h->gamma.p, h->acc.p, s);
    h->last_batch = nc;
    h->pending -= nc;
  }
  if (h->pending == 0 && h->wide_sites) {
    TMH_HIP(hipMemsetAsync(h->wide.p, 0, 16, s));
    h->wide_sites = 0;
  }
  if (cross) defer_join(h, s);
}

// One or several jobs' fused passes in ONE launch (a rank's channels): a short
// job's launch ends with most workgroups idle for a unit's time and starts
// with the pipeline filling; one sweep over every job's units pays that once.
// A job whose configuration differs from the first's gets a launch of its
// own, and a call with a job that needs the two-pass path runs its jobs one
// by one, all on the same stream; results are the per-job calls' in every
// case.
static void correct_hist_multi(tmh_corrector* const* cs, tmh_stats* const* hs, int n_jobs,
                               const uint16_t* const* ins, uint16_t* const* outs,
                               const SiteTab* tabs, const int64_t* n_sites, int clip_lo,
                               int clip_hi, void* stream) {
  TMH_CHECK(cs && hs && n_sites && n_jobs >= 1 && n_jobs <= kMaxJobs, TMH_EINVAL,
            "bad arguments (1 to 8 jobs)");
  check_clip(clip_lo, clip_hi, 65535);
  for (int j = 0; j < n_jobs; ++j) {
    TMH_CHECK(cs[j] && hs[j] && n_sites[j] >= 0, TMH_EINVAL, "bad arguments");
    fused_check(cs[j], hs[j], n_sites[j]);
    TMH_CHECK(cs[j]->npx == cs[0]->npx && cs[j]->log_transform == cs[0]->log_transform,
              TMH_EINVAL, "the jobs of one call need the same image size and transform");
    for (int k = 0; k < j; ++k)
      TMH_CHECK(cs[k] != cs[j] && hs[k] != hs[j], TMH_EINVAL,
                "each job needs its own corrector and statistics handle");
  }
  hipStream_t s = pick(cs[0]->stream, stream);
  bool vec[kMaxJobs], all_vec = true;
  for (int j = 0; j < n_jobs; ++j) {
    vec[j] = fused_vec(cs[j], hs[j], ins ? ins[j] : nullptr, outs ? outs[j] : nullptr, tabs[j]);
    all_vec = all_vec && vec[j];
  }
  if (!all_vec) {
    for (int j = 0; j < n_jobs; ++j) {
      if (n_sites[j] == 0) continue;
      hipStream_t sj = pick(cs[j]->stream, s);
      if (vec[j])
        correct_hist_multi(cs + j, hs + j, 1, ins + j, outs + j, tabs + j, n_sites + j, clip_lo,
                           clip_hi, sj);
      else
        correct_hist_two_pass(cs[j], hs[j], ins[j], outs[j], n_sites[j], clip_lo, clip_hi, sj);
    }
    return;
  }
  FusedPass p[kMaxJobs];
  int np = 0;
  for (int j = 0; j < n_jobs; ++j) {
    if (n_sites[j] == 0) continue;
    const bool cross = fused_begin(cs[j], hs[j], s);
    p[np] = FusedPass{cs[j], hs[j], ins ? ins[j] : nullptr, outs ? outs[j] : nullptr, n_sites[j],
                      tabs[j], s, cross, clip_lo, clip_hi};
    fused_prepare(p[np]);
    ++np;
  }
  if (np == 0) return;
  // every job's fixup counter and unit queues, zeroed by one kernel (a fill
  // per array cost ~10 us each on the pass stream, 8 of them ahead of a
  // four-job launch)
  ZeroList32 Z;
  for (int j = 0; j < np; ++j) {
    Z.add(p[j].c->fix_n.p, 1);
    Z.add(p[j].c->queues.p, kFusedQueueInts);
  }
  launch_zero_u32(Z, s);
  // the jobs of the first job's configuration in one launch, whose unit
  // counters are the first job's queues[0..8); every job's round-mask union
  // is its own corrector's queues + 8
  tmh_corrector* c0 = p[0].c;
  FusedJobs J{};
  for (int j = 0; j < np; ++j) {
    tmh_corrector* c = p[j].c;
    const FusedJob job{p[j].in, p[j].out, p[j].n, reinterpret_cast<const float4*>(c->coef2.p),
                       c->mconst2.p, p[j].fl, p[j].h->hist_full.p, p[j].h->hist_rmask.p,
                       reinterpret_cast<unsigned long long*>(c->queues.p + 8), p[j].tab, p[j].rl};
    if (p[j].cfg == p[0].cfg) {
      J.j[J.n++] = job;
      continue;
    }
    FusedJobs own{};  // another configuration: its own launch
    own.j[own.n++] = job;
    launch_correct_hist(own, c->npx, c->log_transform, clip_lo, clip_hi, c->queues.p, c->n_wg,
                        p[j].cfg, c->bands, s);
  }
  launch_correct_hist(J, c0->npx, c0->log_transform, clip_lo, clip_hi, c0->queues.p, c0->n_wg,
                      p[0].cfg, c0->bands, s);
  // every job's fixups (and Welford wide-counter reset) in one launch
  FixJobs F{};
  for (int j = 0; j < np; ++j) {
    tmh_corrector* c = p[j].c;
    F.j[F.n++] = FixJob{p[j].in, p[j].out, p[j].n, p[j].fl, c->coef64.p, c->rc.p, p[j].tab,
                        p[j].h->pending - p[j].n == 0 ? p[j].h->wide.p : nullptr};
  }
  launch_fix_correct_jobs(F, c0->npx, c0->log_transform, clip_lo, clip_hi, s);
  for (int j = 0; j < np; ++j) fused_post(p[j]);
  // every job's histogram tail (column sums, order statistics) in two
  // launches on one stream: the first job's tail stream when the jobs run
  // off their handles' streams, else s
  bool same_cross = true;
  for (int j = 1; j < np; ++j) same_cross = same_cross && p[j].cross == p[0].cross;
  if (!same_cross) {  // mixed: per-job tails
    for (int j = 0; j < np; ++j) fused_tail(p[j]);
    return;
  }
  hipStream_t ts = fused_tail_stream(p[0]);
  TailJobs T{};
  for (int j = 0; j < np; ++j)
    if (p[j].cfg != kFusedNoHist)  // (very wide: its order statistics are written)
      T.j[T.n++] = tail_job(p[j]);
  launch_hist_finalize_jobs(T, ts);
  for (int j = 0; j < np; ++j) fused_tail_end(p[j], ts);
}

// One job (the single-job entry points): the several-jobs path with one job
static void correct_hist_dev(tmh_corrector* c, tmh_stats* h, const uint16_t* dev_in,
                             uint16_t* dev_out, int64_t n_sites, int clip_lo, int clip_hi,
                             void* stream, const SiteTab& tab) {
  fused_check(c, h, n_sites);
  check_clip(clip_lo, clip_hi, 65535);
  if (n_sites == 0) return;
  correct_hist_multi(&c, &h, 1, &dev_in, &dev_out, &tab, &n_sites, clip_lo, clip_hi, stream);
}

}  // namespace tmh

extern "C" {

int tmh_correct_u16_hist_device(tmh_corrector* c, tmh_stats* h, const uint16_t* dev_in,
                                uint16_t* dev_out, int64_t n_sites, int clip_lo, int clip_hi,
                                void* stream) {
  return guard([&] {
    TMH_CHECK(c && h && (dev_in && dev_out || n_sites == 0) && n_sites >= 0, TMH_EINVAL,
              "bad arguments");
    // the pass re-reads its input after storing outputs (f64 fixups, packed
    // counter recounts): input and output must not overlap
    TMH_CHECK(n_sites == 0 || dev_in + n_sites * h->npx <= dev_out ||
                  dev_out + n_sites * h->npx <= dev_in,
              TMH_EINVAL, "input and output sites must not overlap");
    correct_hist_dev(c, h, dev_in, dev_out, n_sites, clip_lo, clip_hi, stream, SiteTab{});
  });
}

int tmh_correct_u16_hist_blocks_device(tmh_corrector* c, tmh_stats* h,
                                       const uint16_t* const* dev_in_blocks,
                                       uint16_t* const* dev_out_blocks, int block_shift,
                                       int64_t n_sites, int clip_lo, int clip_hi, void* stream) {
  return guard([&] {
    TMH_CHECK(c && h && n_sites >= 0 && dev_out_blocks, TMH_EINVAL, "bad arguments");
    TMH_CHECK(dev_in_blocks != (const uint16_t* const*)dev_out_blocks, TMH_EINVAL,
              "input and output block tables must differ");
    const SiteTab tab = blocked_tab(dev_in_blocks, dev_out_blocks, block_shift, h->npx);
    correct_hist_dev(c, h, nullptr, nullptr, n_sites, clip_lo, clip_hi, stream, tab);
  });
}

int tmh_correct_u16_hist_multi_device(tmh_corrector* const* correctors, tmh_stats* const* handles,
                                      int n_jobs, const uint16_t* const* dev_in,
                                      uint16_t* const* dev_out, const int64_t* n_sites,
                                      int clip_lo, int clip_hi, void* stream) {
  return guard([&] {
    TMH_CHECK(dev_in && dev_out && n_jobs >= 1 && n_jobs <= kMaxJobs && n_sites, TMH_EINVAL,
              "bad arguments");
    SiteTab tabs[kMaxJobs];
    for (int j = 0; j < n_jobs; ++j) {
      TMH_CHECK(n_sites[j] >= 0 && (n_sites[j] == 0 || (dev_in[j] && dev_out[j])), TMH_EINVAL,
                "bad arguments");
      const int64_t npx = handles && handles[j] ? handles[j]->npx : 0;
      TMH_CHECK(n_sites[j] == 0 || dev_in[j] + n_sites[j] * npx <= dev_out[j] ||
                    dev_out[j] + n_sites[j] * npx <= dev_in[j],
                TMH_EINVAL, "input and output sites must not overlap");
    }
    correct_hist_multi(correctors, handles, n_jobs, dev_in, dev_out, tabs, n_sites, clip_lo,
                       clip_hi, stream);
  });
}

int tmh_correct_u16_hist_multi_blocks_device(tmh_corrector* const* correctors,
                                             tmh_stats* const* handles, int n_jobs,
                                             const uint16_t* const* const* dev_in_blocks,
                                             uint16_t* const* const* dev_out_blocks,
                                             int block_shift, const int64_t* n_sites, int clip_lo,
                                             int clip_hi, void* stream) {
  return guard([&] {
    TMH_CHECK(dev_in_blocks && dev_out_blocks && handles && n_jobs >= 1 && n_jobs <= kMaxJobs,
              TMH_EINVAL, "bad arguments");
    SiteTab tabs[kMaxJobs];
    for (int j = 0; j < n_jobs; ++j) {
      TMH_CHECK(handles[j] && dev_out_blocks[j], TMH_EINVAL, "bad arguments");
      TMH_CHECK(dev_in_blocks[j] != (const uint16_t* const*)dev_out_blocks[j], TMH_EINVAL,
                "input and output block tables must differ");
      tabs[j] = blocked_tab(dev_in_blocks[j], dev_out_blocks[j], block_shift, handles[j]->npx);
    }
    correct_hist_multi(correctors, handles, n_jobs, nullptr, nullptr, tabs, n_sites, clip_lo,
                       clip_hi, stream);
  });
}

}  // extern "C"
