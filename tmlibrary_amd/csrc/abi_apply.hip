// C-ABI of libtmhip.so (include/tmhip.h): smoothing, the corrector, plain correction.
#include <cmath>
#include <cstdlib>
#include <map>
#include <mutex>

#include "abi_internal.h"

namespace tmh {

static std::vector<double> gaussian_taps(double sigma) {
  // mahotas 1.4.3 gaussian_filter1d (order 0): radius int(4 sd + 0.5)
  const int lw = (int)(4.0 * sigma + 0.5);
  std::vector<double> w(2 * lw + 1, 0.0);
  w[lw] = 1.0;
  double sum = 1.0;
  const double sd2 = sigma * sigma;
  for (int ii = 1; ii <= lw; ++ii) {
    const double t = std::exp(-0.5 * (double)(ii * ii) / sd2);
    w[lw + ii] = t;
    w[lw - ii] = t;
    sum += 2.0 * t;
  }
  for (auto& x : w) x /= sum;
  return w;
}

// taps per sigma, uploaded once (no allocation or sync on later calls)
static std::mutex g_taps_mu;
static std::map<double, std::pair<double*, int>> g_taps;

static std::pair<double*, int> taps_for(double sigma) {
  std::lock_guard<std::mutex> lk(g_taps_mu);
  auto it = g_taps.find(sigma);
  if (it != g_taps.end()) return it->second;
  const auto w = gaussian_taps(sigma);
  double* d = nullptr;
  TMH_HIP(hipMalloc(&d, w.size() * 8));
  TMH_HIP(hipMemcpy(d, w.data(), w.size() * 8, hipMemcpyHostToDevice));
  auto v = std::make_pair(d, (int)(w.size() / 2));
  g_taps[sigma] = v;
  return v;
}

static void coef_job(CoefJobs& J, int k, tmh_corrector* c, const double* d_mean,
                     const double* d_std) {
  J.mean[k] = d_mean;
  J.std[k] = d_std;
  J.partial[k] = c->partial.p;
  J.sums[k] = c->sums.p;
  // the LUT path's coef and the chain's coef_lin are made when a call needs
  // them (corrector_forms): the fused job path reads only coef2 and coef64
  // (24 of the 48 B/px the full set writes)
  J.coef[k] = nullptr;
  J.coef2[k] = c->coef2.p;
  J.coef_lin[k] = nullptr;
  c->forms_stale = true;
  J.coef64[k] = c->coef64.p;
  J.mconst[k] = c->mconst.p;
  J.mconst2[k] = c->mconst2.p;
  J.rc[k] = c->rc.p;
  J.log_transform[k] = c->log_transform;
  J.zero_log10[k] = c->zero_log10;
}

// coef / coef_lin for the calls that read them, from the last update
void corrector_forms(tmh_corrector* c, hipStream_t s) {
  if (!c->forms_stale) return;
  launch_coeffs_forms(c->coef64.p, c->sums.p, c->npx, c->log_transform, c->coef.p, c->coef_lin.p, s);
  c->forms_stale = false;
}

static void corrector_coeffs(tmh_corrector* c, const double* d_mean, const double* d_std,
                             hipStream_t s) {
  ProfScope prof("coeffs", s);
  CoefJobs J{};
  coef_job(J, 0, c, d_mean, d_std);
  launch_coeffs_jobs(J, 1, c->H, c->W, false, s);
}

static void corrector_init(tmh_corrector* c, const double* d_mean, const double* d_std) {
  c->sums.alloc(3);
  c->partial.alloc(3 * (size_t)coef_tiles(c->H, c->W));
  c->coef.alloc(c->npx);
  c->coef2.alloc(c->npx);
  c->coef_lin.alloc(c->npx);
  c->coef64.alloc(c->npx);
  c->mconst.alloc(1);
  c->mconst2.alloc(1);
  c->rc.alloc(1);
  c->fix_n.alloc(1, true);
  TMH_HIP(hipDeviceGetAttribute(&c->n_wg, hipDeviceAttributeMultiprocessorCount, c->device));
  c->queues.alloc(kFusedQueueInts, true);
  corrector_coeffs(c, d_mean, d_std, c->stream);
}

// The refinement list of one correct launch over n_sites sites on stream s:
// capacity for 1/1024 of the launch's pixels (an overflow makes the fixup
// recompute every pixel in f64: slow but exact).  One launch at a time per
// corrector (the list is reused).  The caller zeroes the count ...
FixList corrector_fixlist(tmh_corrector* c, int64_t n_sites) {
  TMH_CHECK(n_sites < ((int64_t)1 << 24), TMH_EINVAL, "at most 2^24 - 1 sites per correct call");
  const int64_t want = std::min<int64_t>(std::max<int64_t>((int64_t)1 << 20, n_sites * c->npx / 1024),
                                         (int64_t)1 << 30);
  if ((size_t)want > c->fix_e.n) {
    TMH_HIP(hipDeviceSynchronize());  // the list may be in use on any stream
    c->fix_e.alloc((size_t)want);
  }
  return FixList{c->fix_e.p, c->fix_n.p, (unsigned int)c->fix_e.n};
}

// ... or has it reset here, on s
FixList corrector_fixlist(tmh_corrector* c, int64_t n_sites, hipStream_t s) {
  const FixList fl = corrector_fixlist(c, n_sites);
  TMH_HIP(hipMemsetAsync(fl.n, 0, sizeof(unsigned int), s));
  return fl;
}

void check_clip(int lo, int hi, int maxv) {
  if (lo < 0) return;
  TMH_CHECK(lo <= maxv && hi >= 0 && hi <= maxv, TMH_EINVAL, "clip bounds out of range");
}

static void smooth_dev(const double* dev_in, double* dev_out, double* dev_tmp, int height,
                       int width, double sigma, void* stream) {
  TMH_CHECK(dev_in && dev_out && dev_tmp && height > 0 && width > 0, TMH_EINVAL, "bad arguments");
  TMH_CHECK(sigma >= 0.125, TMH_EINVAL, "sigma must be >= 0.125");
  TMH_CHECK(dev_tmp != dev_in && dev_tmp != dev_out, TMH_EINVAL, "dev_tmp must be a third buffer");
  const auto t = taps_for(sigma);
  launch_smooth(dev_in, dev_out, dev_tmp, height, width, t.first, t.second, (hipStream_t)stream);
}

static void corrector_create_dev(const double* dev_mean, const double* dev_std, int height,
                                 int width, int log_transform, double zero_log10, void* stream,
                                 tmh_corrector** out) {
  TMH_CHECK(out && dev_mean && dev_std && height > 0 && width > 0, TMH_EINVAL, "bad arguments");
  auto* c = new tmh_corrector();
  try {
    TMH_HIP(hipGetDevice(&c->device));
    c->H = height;
    c->W = width;
    c->npx = (int64_t)height * width;
    c->log_transform = log_transform ? 1 : 0;
    c->zero_log10 = zero_log10;
    c->stream = (hipStream_t)stream;
    c->lut.alloc(kBins);
    launch_build_corr_lut(c->lut.p, c->log_transform, zero_log10, c->stream);
    corrector_init(c, dev_mean, dev_std);
  } catch (...) {
    delete c;
    throw;
  }
  *out = c;
}

}  // namespace tmh

extern "C" {

int tmh_smooth_f64_device(const double* dev_in, double* dev_out, double* dev_tmp, int height,
                          int width, double sigma, void* stream) {
  return guard([&] { smooth_dev(dev_in, dev_out, dev_tmp, height, width, sigma, stream); });
}

int tmh_smooth2_f64_device(const double* dev_in0, const double* dev_in1, double* dev_out0,
                           double* dev_out1, double* dev_tmp0, double* dev_tmp1, int height,
                           int width, double sigma, void* stream) {
  return guard([&] {
    TMH_CHECK(dev_in0 && dev_in1 && dev_out0 && dev_out1 && dev_tmp0 && dev_tmp1 && height > 0 &&
                  width > 0,
              TMH_EINVAL, "bad arguments");
    TMH_CHECK(sigma >= 0.125, TMH_EINVAL, "sigma must be >= 0.125");
    const double* ins[2] = {dev_in0, dev_in1};
    const double* outs[2] = {dev_out0, dev_out1};
    for (const double* t : {(const double*)dev_tmp0, (const double*)dev_tmp1})
      for (int k = 0; k < 2; ++k)
        TMH_CHECK(t != ins[k] && t != outs[k], TMH_EINVAL, "dev_tmp0/1 must be buffers of their own");
    TMH_CHECK(dev_tmp0 != dev_tmp1, TMH_EINVAL, "dev_tmp0 and dev_tmp1 must differ");
    TMH_CHECK(dev_out0 != dev_out1, TMH_EINVAL, "dev_out0 and dev_out1 must differ");
    const auto t = taps_for(sigma);
    launch_smooth2(dev_in0, dev_in1, dev_out0, dev_out1, dev_tmp0, dev_tmp1, height, width,
                   t.first, t.second, (hipStream_t)stream);
  });
}

int tmh_smooth_f64(const double* host_in, double* host_out, int height, int width, double sigma) {
  return guard([&] {
    TMH_CHECK(host_in && host_out && height > 0 && width > 0, TMH_EINVAL, "bad arguments");
    const size_t npx = (size_t)height * width;
    DBuf<double> a, b, t;
    a.upload(host_in, npx);
    b.alloc(npx);
    t.alloc(npx);
    smooth_dev(a.p, b.p, t.p, height, width, sigma, nullptr);
    TMH_HIP(hipDeviceSynchronize());
    b.download(host_out, npx);
  });
}

int tmh_corrector_create_device(const double* dev_mean, const double* dev_std, int height,
                                int width, int log_transform, double zero_log10, void* stream,
                                tmh_corrector** out) {
  return guard([&] {
    corrector_create_dev(dev_mean, dev_std, height, width, log_transform, zero_log10, stream, out);
  });
}

int tmh_corrector_create(const double* host_mean, const double* host_std, int height, int width,
                         int log_transform, double zero_log10, tmh_corrector** out) {
  return guard([&] {
    TMH_CHECK(out && host_mean && host_std && height > 0 && width > 0, TMH_EINVAL, "bad arguments");
    const size_t npx = (size_t)height * width;
    DBuf<double> m, s;
    m.upload(host_mean, npx);
    s.upload(host_std, npx);
    corrector_create_dev(m.p, s.p, height, width, log_transform, zero_log10, nullptr, out);
    TMH_HIP(hipDeviceSynchronize());
  });
}

void tmh_corrector_destroy(tmh_corrector* c) {
  if (!c) return;
  (void)hipStreamSynchronize(c->stream);
  if (c->ev_tail) {
    (void)hipEventSynchronize(c->ev_tail);
    (void)hipEventDestroy(c->ev_tail);
  }
  delete c;
}

int tmh_corrector_set_option(tmh_corrector* c, int option, int value) {
  return guard([&] {
    TMH_CHECK(c, TMH_EINVAL, "corrector is NULL");
    if (option == TMH_OPT_FUSED_BANDS) {
      TMH_CHECK(value == 0 || value == 8 || value == 16 || value == 32 || value == 64, TMH_EINVAL,
                "fused bands must be 0 (automatic), 8, 16, 32 or 64");
      c->bands = value;
      return;
    }
    if (option == TMH_OPT_FUSED_CUS) {
      int cus = 256;
      TMH_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->device));
      TMH_CHECK(value >= 0 && value <= cus, TMH_EINVAL, "fused CUs must be 0..CU count");
      c->n_wg = value ? value : cus;
      return;
    }
    if (!c->host.set(option, value)) throw Error{TMH_EINVAL, "unknown corrector option"};
  });
}

int tmh_corrector_update_device(tmh_corrector* c, const double* dev_mean, const double* dev_std,
                                void* stream) {
  return guard([&] {
    TMH_CHECK(c && dev_mean && dev_std, TMH_EINVAL, "bad arguments");
    corrector_coeffs(c, dev_mean, dev_std, pick(c->stream, stream));
  });
}

int tmh_corrector_update_multi_device(tmh_corrector* const* cs, int n, const double* const* dev_mean,
                                      const double* const* dev_std, void* stream) {
  return guard([&] {
    TMH_CHECK(cs && dev_mean && dev_std && n >= 1 && n <= kMaxJobs, TMH_EINVAL,
              "bad arguments (1 <= n <= 8 correctors)");
    CoefJobs J{};
    for (int k = 0; k < n; ++k) {
      TMH_CHECK(cs[k] && dev_mean[k] && dev_std[k], TMH_EINVAL, "bad arguments");
      TMH_CHECK(cs[k]->npx == cs[0]->npx, TMH_EINVAL, "correctors of different image sizes");
      coef_job(J, k, cs[k], dev_mean[k], dev_std[k]);
    }
    for (int k = 0; k < n; ++k)
      TMH_CHECK(cs[k]->H == cs[0]->H && cs[k]->W == cs[0]->W, TMH_EINVAL,
                "correctors of different image shapes");
    const hipStream_t s = pick(cs[0]->stream, stream);
    ProfScope prof("coeffs", s);
    launch_coeffs_jobs(J, n, cs[0]->H, cs[0]->W, false, s);
  });
}

int tmh_job_planes_multi_device(tmh_stats* const* hs, tmh_corrector* const* cs, int n,
                                double* const* dev_mean, double* const* dev_std,
                                double* const* dev_smean, double* const* dev_sstd, double sigma,
                                void* stream) {
  return guard([&] {
    TMH_CHECK(hs && cs && dev_smean && dev_sstd && n >= 1 && n <= kMaxJobs, TMH_EINVAL,
              "bad arguments (1 <= n <= 8 jobs)");
    TMH_CHECK(sigma >= 0.125, TMH_EINVAL, "sigma must be >= 0.125");
    for (int k = 0; k < n; ++k) {
      TMH_CHECK(hs[k] && cs[k] && dev_smean[k] && dev_sstd[k], TMH_EINVAL, "bad arguments");
      TMH_CHECK(hs[k]->H == hs[0]->H && hs[k]->W == hs[0]->W && cs[k]->npx == hs[0]->npx,
                TMH_EINVAL, "jobs of different image sizes");
      // (every check before the first cross_begin / launch: a rejected call
      // leaves nothing queued that reads scratch freed on the way out)
      TMH_CHECK(cs[k]->H == hs[0]->H && cs[k]->W == hs[0]->W, TMH_EINVAL,
                "jobs of different image shapes");
      TMH_CHECK(dev_smean[k] != dev_sstd[k], TMH_EINVAL, "smoothed planes must differ");
      for (int j = 0; j < k; ++j)
        TMH_CHECK(hs[j] != hs[k] && cs[j] != cs[k], TMH_EINVAL, "a handle listed twice");
    }
    const int H = hs[0]->H, W = hs[0]->W;
    const int64_t npx = hs[0]->npx;
    const hipStream_t s = pick(hs[0]->stream, stream);
    for (int k = 0; k < n; ++k) cross_begin(hs[k], s);
    // stats.py:94-112 as asked for (the unsmoothed planes: what the
    // illumstats file keeps); the smoothing reads the handles' state itself
    for (int k = 0; k < n; ++k) {
      const bool m = dev_mean && dev_mean[k], d = dev_std && dev_std[k];
      if (m || d)
        launch_finalize(hs[k]->mean.p, hs[k]->m2.p, hs[k]->n, npx, m ? dev_mean[k] : nullptr,
                        d ? dev_std[k] : nullptr, s);
    }
    // IllumstatsContainer.smooth (image.py:1172-1193), every job's mean and
    // std in one launch; the std planes finalized as they are read
    const auto t = taps_for(sigma);
    const double* in[kMaxPlanes];
    double* out[kMaxPlanes];
    double sq[kMaxPlanes];
    DBuf<double> scratch;
    const bool onepass = t.second == 20 && W >= 41 && !getenv("TMH_SMOOTH_2PASS");
    if (!onepass) scratch.alloc((size_t)3 * n * npx);  // finalized std + axis-0 temps
    double* tmp[kMaxPlanes];
    for (int k = 0; k < n; ++k) {
      tmh_stats* h = hs[k];
      in[2 * k] = h->mean.p;
      out[2 * k] = dev_smean[k];
      sq[2 * k] = 0.0;
      out[2 * k + 1] = dev_sstd[k];
      if (onepass) {
        in[2 * k + 1] = h->m2.p;
        sq[2 * k + 1] = h->n >= 2 ? (double)(h->n - 1) : -1.0;
      } else {
        double* sd = scratch.p + (size_t)(3 * k) * npx;
        launch_finalize(h->mean.p, h->m2.p, h->n, npx, nullptr, sd, s);
        in[2 * k + 1] = sd;
        sq[2 * k + 1] = 0.0;
        tmp[2 * k] = scratch.p + (size_t)(3 * k + 1) * npx;
        tmp[2 * k + 1] = scratch.p + (size_t)(3 * k + 2) * npx;
      }
    }
    // the coefficient tiles' sums of the smoothed planes come with them
    // (psum / pmin: std sums, mean sums, std minima in each corrector's
    // partial buffer)
    const int nt = coef_tiles(H, W);
    double* psum[kMaxPlanes];
    double* pmin[kMaxPlanes];
    for (int k = 0; k < n; ++k) {
      psum[2 * k] = cs[k]->partial.p + nt;  // mean
      pmin[2 * k] = nullptr;
      psum[2 * k + 1] = cs[k]->partial.p;  // std
      pmin[2 * k + 1] = cs[k]->partial.p + 2 * nt;
    }
    launch_smooth_planes(in, out, onepass ? out : tmp, sq, 2 * n, H, W, t.first, t.second, s,
                         psum, pmin);
    // the correctors' coefficients (image.py:599-631) from the smoothed planes
    CoefJobs J{};
    for (int k = 0; k < n; ++k) coef_job(J, k, cs[k], dev_smean[k], dev_sstd[k]);
    {
      ProfScope prof("coeffs", s);
      launch_coeffs_jobs(J, n, H, W, true, s);
    }
    for (int k = 0; k < n; ++k) cross_end(hs[k], s);
    if (!onepass) TMH_HIP(hipStreamSynchronize(s));  // the scratch is freed on return
  });
}

int tmh_corrector_means(tmh_corrector* c, double* mean_of_std, double* mean_of_mean) {
  return guard([&] {
    TMH_CHECK(c, TMH_EINVAL, "corrector is NULL");
    double sums[2];
    TMH_HIP(hipStreamSynchronize(c->stream));
    TMH_HIP(hipMemcpy(sums, c->sums.p, 16, hipMemcpyDeviceToHost));
    if (mean_of_std) *mean_of_std = sums[0] / (double)c->npx;
    if (mean_of_mean) *mean_of_mean = sums[1] / (double)c->npx;
  });
}

int tmh_correct_u16_device(tmh_corrector* c, const uint16_t* dev_in, uint16_t* dev_out,
                           int64_t n_sites, int clip_lo, int clip_hi, void* stream) {
  return guard([&] {
    TMH_CHECK(c && (dev_in && dev_out || n_sites == 0) && n_sites >= 0, TMH_EINVAL, "bad arguments");
    check_clip(clip_lo, clip_hi, 65535);
    // the f64 fixup re-reads the input after the streaming kernel has stored
    // the output: input and output must not overlap
    TMH_CHECK(n_sites == 0 || dev_in + n_sites * c->npx <= dev_out ||
                  dev_out + n_sites * c->npx <= dev_in,
              TMH_EINVAL, "input and output sites must not overlap");
    hipStream_t s = pick(c->stream, stream);
    const FixList fl = corrector_fixlist(c, n_sites, s);
    corrector_forms(c, s);
    launch_correct_u16(dev_in, dev_out, c->npx, n_sites, c->coef.p, c->lut.p, c->mconst.p, fl,
                       c->log_transform, clip_lo, clip_hi, s);
    launch_fix_correct(dev_in, dev_out, 2, c->npx, n_sites, fl, c->coef64.p, c->rc.p,
                       c->log_transform, clip_lo, clip_hi, s);
  });
}

int tmh_correct_u16(tmh_corrector* c, const uint16_t* host_in, uint16_t* host_out, int64_t n_sites,
                    int clip_lo, int clip_hi) {
  return guard([&] {
    TMH_CHECK(c && (host_in && host_out || n_sites == 0) && n_sites >= 0, TMH_EINVAL,
              "bad arguments");
    check_clip(clip_lo, clip_hi, 65535);
    if (n_sites == 0) return;
    // chunks of <= 16 sites (~177 MB at 2160x2560), two slots per direction
    const int64_t step =
        std::max<int64_t>(1, std::min<int64_t>({16, n_sites, ((int64_t)192 << 20) / (c->npx * 2)}));
    const size_t slot_px = (size_t)step * c->npx;
    if (2 * slot_px > c->stage_in.n) {
      TMH_HIP(hipStreamSynchronize(c->stream));
      c->stage_in.ensure(2 * slot_px);
      c->stage_out.ensure(2 * slot_px);
    }
    HostPipe& p = c->pipe;
    p.init();
    auto retire = [&](int slot) {
      if (!p.busy[slot]) return;
      TMH_HIP(hipEventSynchronize(p.ev_done[slot]));
      par_copy(host_out + p.s0[slot] * c->npx, p.out[slot].p, (size_t)p.ns[slot] * c->npx * 2,
               c->host.copy_threads);
      p.busy[slot] = false;
    };
    int64_t k = 0;
    try {
      for (int64_t s0 = 0; s0 < n_sites; s0 += step, ++k) {
        const int slot = (int)(k & 1);
        const int64_t ns = std::min(step, n_sites - s0);
        const size_t bytes = (size_t)ns * c->npx * 2;
        retire(slot);  // chunk k-2: output copied out, both slot buffers free
        p.out[slot].ensure(slot_px * 2);
        uint16_t* din = c->stage_in.p + (size_t)slot * slot_px;
        uint16_t* dout = c->stage_out.p + (size_t)slot * slot_px;
        TMH_HIP(hipMemcpyAsync(din, host_in + s0 * c->npx, bytes, hipMemcpyHostToDevice, p.h2d));
        TMH_HIP(hipEventRecord(p.ev_in[slot], p.h2d));
        TMH_HIP(hipStreamWaitEvent(c->stream, p.ev_in[slot], 0));
        const FixList fl = corrector_fixlist(c, ns, c->stream);
        corrector_forms(c, c->stream);
        launch_correct_u16(din, dout, c->npx, ns, c->coef.p, c->lut.p, c->mconst.p, fl,
                           c->log_transform, clip_lo, clip_hi, c->stream);
        launch_fix_correct(din, dout, 2, c->npx, ns, fl, c->coef64.p, c->rc.p, c->log_transform,
                           clip_lo, clip_hi, c->stream);
        TMH_HIP(hipEventRecord(p.ev_kern[slot], c->stream));
        TMH_HIP(hipStreamWaitEvent(p.d2h, p.ev_kern[slot], 0));
        TMH_HIP(hipMemcpyAsync(p.out[slot].p, dout, bytes, hipMemcpyDeviceToHost, p.d2h));
        TMH_HIP(hipEventRecord(p.ev_done[slot], p.d2h));
        p.busy[slot] = true;
        p.s0[slot] = s0;
        p.ns[slot] = ns;
      }
      retire((int)(k & 1));
      retire((int)((k + 1) & 1));
    } catch (...) {
      p.abandon(c->stream);
      throw;
    }
  });
}

int tmh_correct_u8(tmh_corrector* c, const uint8_t* host_in, uint8_t* host_out, int64_t n_sites,
                   int clip_lo, int clip_hi) {
  return guard([&] {
    TMH_CHECK(c && (host_in && host_out || n_sites == 0) && n_sites >= 0, TMH_EINVAL,
              "bad arguments");
    check_clip(clip_lo, clip_hi, 255);
    const size_t bytes = (size_t)n_sites * c->npx;
    if (!bytes) return;
    c->stage8_in.ensure(bytes);
    c->stage8_out.ensure(bytes);
    TMH_HIP(hipMemcpyAsync(c->stage8_in.p, host_in, bytes, hipMemcpyHostToDevice, c->stream));
    const FixList fl = corrector_fixlist(c, n_sites, c->stream);
    corrector_forms(c, c->stream);
    launch_correct_u8(c->stage8_in.p, c->stage8_out.p, c->npx, n_sites, c->coef.p, c->lut.p,
                      c->mconst.p, fl, c->log_transform, clip_lo, clip_hi, c->stream);
    launch_fix_correct(c->stage8_in.p, c->stage8_out.p, 1, c->npx, n_sites, fl, c->coef64.p,
                       c->rc.p, c->log_transform, clip_lo, clip_hi, c->stream);
    TMH_HIP(hipMemcpyAsync(host_out, c->stage8_out.p, bytes, hipMemcpyDeviceToHost, c->stream));
    TMH_HIP(hipStreamSynchronize(c->stream));
  });
}

}  // extern "C"
