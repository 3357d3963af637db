// C-ABI of libtmhip.so (include/tmhip.h): the clustering tool -- column census
// and order statistics (RobustScaler), robust scaling, k-means++ seeding,
// k-means predict and fit.
#include <climits>
#include <cmath>

#include "abi_internal.h"

namespace tmh {

void check_table(const void* x, int64_t n, int d) {
  TMH_CHECK(x, TMH_EINVAL, "data pointer is NULL");
  TMH_CHECK(n >= 1 && n < ((int64_t)1 << 31), TMH_EINVAL, "n must be 1 .. 2^31 - 1 rows");
  TMH_CHECK(d >= 1 && d <= TMH_CLUSTER_MAX_D, TMH_EINVAL, "d is over the limit of 256 features");
  TMH_CHECK((reinterpret_cast<uintptr_t>(x) & 7) == 0, TMH_EINVAL, "data must be 8-byte aligned");
}

void check_scaler(const double* center, const double* scale) {
  TMH_CHECK((center == nullptr) == (scale == nullptr), TMH_EINVAL,
            "center and scale are given together or not at all");
}

// fit and seed pick k rows as centres, so they need k <= n; predict labels any
// number of rows
static void check_kmeans(const void* x, int64_t n, int d, int k, bool needs_k_rows = true) {
  check_table(x, n, d);
  TMH_CHECK(k >= 1 && k <= TMH_CLUSTER_MAX_K, TMH_EINVAL, "k is over the limit of 64 clusters");
  TMH_CHECK((int64_t)k * d <= TMH_CLUSTER_MAX_KD, TMH_EINVAL, "k * d is over the limit of 8,192");
  TMH_CHECK(!needs_k_rows || k <= n, TMH_EINVAL, "more clusters than rows");
}

bool overlap(const void* a, size_t a_bytes, const void* b, size_t b_bytes) {
  const char* pa = static_cast<const char*>(a);
  const char* pb = static_cast<const char*>(b);
  return pa < pb + b_bytes && pb < pa + a_bytes;
}

// counts of the table on the host: cnt[f] non-NaN, cnt[d + f] +-inf (waits)
static std::vector<unsigned long long> census_host(const double* dev_x, int64_t n, int d,
                                                   DBuf<unsigned long long>& cnt, hipStream_t s) {
  cnt.alloc(2 * (size_t)d);
  cluster_census(dev_x, n, d, cnt.p, s);
  std::vector<unsigned long long> h(2 * (size_t)d);
  TMH_HIP(hipMemcpyAsync(h.data(), cnt.p, h.size() * sizeof(unsigned long long),
                         hipMemcpyDeviceToHost, s));
  TMH_HIP(hipStreamSynchronize(s));
  return h;
}

void require_finite(const double* dev_x, int64_t n, int d, DBuf<unsigned long long>& cnt,
                    hipStream_t s) {
  const std::vector<unsigned long long> h = census_host(dev_x, n, d, cnt, s);
  for (int f = 0; f < d; ++f)
    TMH_CHECK(h[(size_t)f] == (unsigned long long)n && h[(size_t)d + f] == 0, TMH_EINVAL,
              "the data holds NaN or infinite values");
}

static void census_dev(const double* dev_x, int64_t n, int d, const double* dev_center,
                       const double* dev_scale, int64_t* host_count, int64_t* host_inf,
                       double* host_mean, double* host_var, void* stream) {
  check_table(dev_x, n, d);
  check_scaler(dev_center, dev_scale);
  TMH_CHECK(host_count && host_inf, TMH_EINVAL, "count pointer is NULL");
  hipStream_t s = (hipStream_t)stream;
  ProfScope prof("column_census", s);
  DBuf<unsigned long long> cnt;
  const std::vector<unsigned long long> h = census_host(dev_x, n, d, cnt, s);
  for (int f = 0; f < d; ++f) {
    host_count[f] = (int64_t)h[(size_t)f];
    host_inf[f] = (int64_t)h[(size_t)d + f];
  }
  if (!host_mean && !host_var) return;
  DBuf<double> part, mv;
  part.alloc((size_t)cluster_colsum_chunks(n) * d);
  mv.alloc(2 * (size_t)d);
  cluster_colstat(dev_x, n, d, dev_center, dev_scale, cnt.p, nullptr, part.p, mv.p, s);
  cluster_colstat(dev_x, n, d, dev_center, dev_scale, cnt.p, mv.p, part.p, mv.p + d, s);
  std::vector<double> out(2 * (size_t)d);
  TMH_HIP(hipMemcpyAsync(out.data(), mv.p, out.size() * sizeof(double), hipMemcpyDeviceToHost, s));
  TMH_HIP(hipStreamSynchronize(s));
  for (int f = 0; f < d; ++f) {
    if (host_mean) host_mean[f] = out[(size_t)f];
    if (host_var) host_var[f] = out[(size_t)d + f];
  }
}

static void select_dev(const double* dev_x, int64_t n, int d, const int64_t* host_count,
                       const int64_t* host_ranks, int r, double* host_values, void* stream) {
  check_table(dev_x, n, d);
  TMH_CHECK(r >= 1 && r <= TMH_CLUSTER_MAX_RANKS, TMH_EINVAL, "r must be 1 .. 64 ranks per column");
  TMH_CHECK(host_ranks && host_values, TMH_EINVAL, "ranks or values pointer is NULL");
  hipStream_t s = (hipStream_t)stream;
  // the ranks are checked against the columns' non-NaN counts: the caller's
  // (tmh_column_census's result), or a census of its own
  std::vector<unsigned long long> h;
  if (host_count) {
    h.resize((size_t)d);
    for (int f = 0; f < d; ++f) {
      TMH_CHECK(host_count[f] >= 0 && host_count[f] <= n, TMH_EINVAL, "a count is outside 0 .. n");
      h[(size_t)f] = (unsigned long long)host_count[f];
    }
  } else {
    DBuf<unsigned long long> cnt;
    h = census_host(dev_x, n, d, cnt, s);
  }
  const size_t tabs = (size_t)d * r;
  std::vector<unsigned long long> st(2 * tabs);
  for (int f = 0; f < d; ++f)
    for (int q = 0; q < r; ++q) {
      const int64_t rank = host_ranks[(size_t)f * r + q];
      TMH_CHECK(rank >= 0 && (unsigned long long)rank < h[(size_t)f], TMH_EINVAL,
                "a rank is outside the column's non-NaN values");
      st[2 * ((size_t)f * r + q)] = 0ull;
      st[2 * ((size_t)f * r + q) + 1] = (unsigned long long)rank;
    }
  DBuf<unsigned long long> state;
  DBuf<unsigned int> hist;
  DBuf<double> out;
  state.alloc(2 * tabs);
  hist.alloc(tabs * 256);
  out.alloc(tabs);
  TMH_HIP(hipMemcpyAsync(state.p, st.data(), st.size() * sizeof(unsigned long long),
                         hipMemcpyHostToDevice, s));
  cluster_select(dev_x, n, d, r, state.p, hist.p, out.p, s);
  TMH_HIP(hipMemcpyAsync(host_values, out.p, tabs * sizeof(double), hipMemcpyDeviceToHost, s));
  TMH_HIP(hipStreamSynchronize(s));
}

static void robust_scale_dev(const double* dev_x, int64_t n, int d, const double* dev_center,
                             const double* dev_scale, double* dev_out, void* stream) {
  check_table(dev_x, n, d);
  TMH_CHECK(dev_center && dev_scale && dev_out, TMH_EINVAL, "center, scale or out pointer is NULL");
  const size_t bytes = (size_t)n * d * sizeof(double);
  TMH_CHECK(!overlap(dev_x, bytes, dev_out, bytes), TMH_EINVAL, "input and output must not overlap");
  cluster_robust_scale(dev_x, n, d, dev_center, dev_scale, dev_out, (hipStream_t)stream);
}

static void predict_dev(const double* dev_x, int64_t n, int d, int k, const double* dev_center,
                        const double* dev_scale, const double* host_centers, int32_t* dev_labels,
                        double* dev_min_dist, void* stream) {
  check_kmeans(dev_x, n, d, k, false);
  check_scaler(dev_center, dev_scale);
  TMH_CHECK(host_centers && dev_labels, TMH_EINVAL, "centers or labels pointer is NULL");
  const size_t xb = (size_t)n * d * sizeof(double);
  TMH_CHECK(!overlap(dev_x, xb, dev_labels, (size_t)n * 4) &&
                (!dev_min_dist || !overlap(dev_x, xb, dev_min_dist, (size_t)n * 8)),
            TMH_EINVAL, "input and output must not overlap");
  for (int i = 0; i < k * d; ++i)
    TMH_CHECK(std::isfinite(host_centers[i]), TMH_EINVAL, "the centers hold NaN or infinite values");
  hipStream_t s = (hipStream_t)stream;
  DBuf<unsigned long long> cnt;
  require_finite(dev_x, n, d, cnt, s);
  DBuf<double> cent;
  cent.alloc((size_t)k * d);
  TMH_HIP(hipMemcpyAsync(cent.p, host_centers, (size_t)k * d * sizeof(double), hipMemcpyHostToDevice,
                         s));
  cluster_assign(dev_x, n, d, k, dev_center, dev_scale, cent.p, nullptr, dev_labels, dev_min_dist,
                 nullptr, nullptr, nullptr, s);
  TMH_HIP(hipStreamSynchronize(s));  // the centres are freed on return
}

static void fit_dev(const double* dev_x, int64_t n, int d, int k, const double* dev_center,
                    const double* dev_scale, const double* host_init, int max_iter, double tol,
                    double* host_centers, int32_t* dev_labels, double* inertia, int* n_iter,
                    double* tol_abs, void* stream) {
  check_kmeans(dev_x, n, d, k);
  check_scaler(dev_center, dev_scale);
  TMH_CHECK(host_init && host_centers && dev_labels && inertia && n_iter && tol_abs, TMH_EINVAL,
            "a centers, labels or result pointer is NULL");
  TMH_CHECK(max_iter >= 1, TMH_EINVAL, "max_iter must be at least 1");
  TMH_CHECK(tol >= 0.0, TMH_EINVAL, "tol must not be negative");
  TMH_CHECK(!overlap(dev_x, (size_t)n * d * sizeof(double), dev_labels, (size_t)n * 4), TMH_EINVAL,
            "input and output must not overlap");
  for (int i = 0; i < k * d; ++i)
    TMH_CHECK(std::isfinite(host_init[i]), TMH_EINVAL, "the centers hold NaN or infinite values");
  hipStream_t s = (hipStream_t)stream;
  DBuf<unsigned long long> cnt;
  require_finite(dev_x, n, d, cnt, s);

  const size_t kd = (size_t)k * d;
  const int64_t chunks = cluster_assign_chunks(n, d, k);
  DBuf<double> cent, mind, psums, sums, small, part, colpart, mv;
  DBuf<unsigned int> pcounts;
  DBuf<long long> counts;
  DBuf<int64_t> taken;
  DBuf<int32_t> lab;
  DBuf<int> changed;
  cent.alloc(2 * kd);
  mind.alloc((size_t)n);
  psums.alloc((size_t)chunks * kd);
  pcounts.alloc((size_t)chunks * k);
  sums.alloc(kd);
  counts.alloc((size_t)k);
  taken.alloc((size_t)k);
  lab.alloc(2 * (size_t)n);
  changed.alloc(1);
  small.alloc(2);  // centre shift, inertia
  part.alloc((size_t)cluster_sum_chunks(n));

  // tol_abs = tol * mean of the column variances of the scaled data
  colpart.alloc((size_t)cluster_colsum_chunks(n) * d);
  mv.alloc(2 * (size_t)d);
  cluster_colstat(dev_x, n, d, dev_center, dev_scale, cnt.p, nullptr, colpart.p, mv.p, s);
  cluster_colstat(dev_x, n, d, dev_center, dev_scale, cnt.p, mv.p, colpart.p, mv.p + d, s);
  std::vector<double> var((size_t)d);
  TMH_HIP(hipMemcpyAsync(var.data(), mv.p + d, (size_t)d * sizeof(double), hipMemcpyDeviceToHost, s));
  TMH_HIP(hipMemcpyAsync(cent.p, host_init, kd * sizeof(double), hipMemcpyHostToDevice, s));
  TMH_HIP(hipStreamSynchronize(s));
  double vsum = 0.0;
  for (int f = 0; f < d; ++f) vsum += var[(size_t)f];
  *tol_abs = tol * (vsum / d);

  double* cur = cent.p;
  double* nxt = cent.p + kd;
  int32_t* lcur = lab.p;
  int32_t* lprev = lab.p + n;
  bool strict = false;
  int it = 0;
  for (int i = 0; i < max_iter; ++i) {
    const bool have_prev = i > 0;
    cluster_assign(dev_x, n, d, k, dev_center, dev_scale, cur, have_prev ? lprev : nullptr, lcur,
                   mind.p, have_prev ? changed.p : nullptr, psums.p, pcounts.p, s);
    cluster_update(dev_x, n, d, k, dev_center, dev_scale, lcur, mind.p, psums.p, pcounts.p, sums.p,
                   counts.p, cur, nxt, small.p, taken.p, s);
    std::swap(cur, nxt);
    int h_changed = 1;
    double h_shift = 0.0;
    if (have_prev)
      TMH_HIP(hipMemcpyAsync(&h_changed, changed.p, sizeof(int), hipMemcpyDeviceToHost, s));
    TMH_HIP(hipMemcpyAsync(&h_shift, small.p, sizeof(double), hipMemcpyDeviceToHost, s));
    TMH_HIP(hipStreamSynchronize(s));
    it = i + 1;
    if (!h_changed) {
      strict = true;
      break;
    }
    if (h_shift <= *tol_abs) break;
    std::swap(lcur, lprev);
  }
  if (strict) {
    TMH_HIP(hipMemcpyAsync(dev_labels, lcur, (size_t)n * 4, hipMemcpyDeviceToDevice, s));
  } else {
    // the labels of the final centres
    cluster_assign(dev_x, n, d, k, dev_center, dev_scale, cur, nullptr, dev_labels, mind.p, nullptr,
                   nullptr, nullptr, s);
  }
  cluster_sum(mind.p, n, 1, part.p, small.p + 1, s);
  TMH_HIP(hipMemcpyAsync(inertia, small.p + 1, sizeof(double), hipMemcpyDeviceToHost, s));
  TMH_HIP(hipMemcpyAsync(host_centers, cur, kd * sizeof(double), hipMemcpyDeviceToHost, s));
  TMH_HIP(hipStreamSynchronize(s));
  *n_iter = it;
}

static void seed_dev(const double* dev_x, int64_t n, int d, int k, const double* dev_center,
                     const double* dev_scale, int64_t first, const double* host_draws, int trials,
                     int32_t* host_indices, double* host_centers, double* host_trace, void* stream) {
  check_kmeans(dev_x, n, d, k);
  check_scaler(dev_center, dev_scale);
  TMH_CHECK(first >= 0 && first < n, TMH_EINVAL, "the first index is outside the rows");
  TMH_CHECK(trials >= 1 && trials <= TMH_CLUSTER_MAX_TRIALS, TMH_EINVAL,
            "trials must be 1 .. 16");
  TMH_CHECK(host_indices && host_centers && (k == 1 || host_draws), TMH_EINVAL,
            "draws, indices or centers pointer is NULL");
  for (int i = 0; i < (k - 1) * trials; ++i)
    TMH_CHECK(host_draws[i] >= 0.0 && host_draws[i] <= 1.0, TMH_EINVAL,
              "a draw is outside [0, 1]");
  hipStream_t s = (hipStream_t)stream;
  DBuf<unsigned long long> cnt;
  require_finite(dev_x, n, d, cnt, s);
  ProfScope prof("kmeans_seed", s);
  const int64_t nb = cluster_seed_blocks(n);
  const int64_t chunks = cluster_sum_chunks(n);
  const size_t tr_len = (size_t)(3 * trials + 1);
  DBuf<double> closest, trial, btot, bexcl, part, pots, pot, targets, draws, cent, trace;
  DBuf<int64_t> cand;
  DBuf<int> best;
  DBuf<int32_t> indices;
  closest.alloc((size_t)n);
  trial.alloc((size_t)n * trials);
  btot.alloc((size_t)nb);
  bexcl.alloc((size_t)nb + 1);
  part.alloc((size_t)chunks * trials);
  pots.alloc((size_t)trials);
  pot.alloc(1);
  targets.alloc((size_t)trials);
  cand.alloc((size_t)trials);
  best.alloc(1);
  indices.alloc((size_t)k);
  cent.alloc((size_t)k * d);
  if (k > 1) {
    draws.upload(host_draws, (size_t)(k - 1) * trials);
    if (host_trace) trace.alloc((size_t)(k - 1) * tr_len);
  }
  const int32_t first32 = (int32_t)first;
  TMH_HIP(hipMemcpyAsync(cand.p, &first, sizeof(int64_t), hipMemcpyHostToDevice, s));
  TMH_HIP(hipMemcpyAsync(indices.p, &first32, sizeof(int32_t), hipMemcpyHostToDevice, s));
  cluster_seed_trials(dev_x, n, d, 1, dev_center, dev_scale, cand.p, nullptr, closest.p, s);
  cluster_sum(closest.p, n, 1, part.p, pot.p, s);
  for (int step = 1; step < k; ++step) {
    cluster_seed_search(closest.p, n, trials, draws.p + (size_t)(step - 1) * trials, pot.p, btot.p,
                        bexcl.p, targets.p, cand.p, s);
    cluster_seed_trials(dev_x, n, d, trials, dev_center, dev_scale, cand.p, closest.p, trial.p, s);
    cluster_sum(trial.p, n, trials, part.p, pots.p, s);
    cluster_seed_pick(pots.p, trials, cand.p, targets.p, step, pot.p, best.p, indices.p, trace.p,
                      trials, trial.p, n, closest.p, s);
  }
  cluster_gather_rows(dev_x, d, k, dev_center, dev_scale, indices.p, cent.p, s);
  TMH_HIP(hipMemcpyAsync(host_indices, indices.p, (size_t)k * 4, hipMemcpyDeviceToHost, s));
  TMH_HIP(hipMemcpyAsync(host_centers, cent.p, (size_t)k * d * 8, hipMemcpyDeviceToHost, s));
  if (host_trace && k > 1)
    TMH_HIP(hipMemcpyAsync(host_trace, trace.p, (size_t)(k - 1) * tr_len * 8, hipMemcpyDeviceToHost,
                           s));
  TMH_HIP(hipStreamSynchronize(s));
}

}  // namespace tmh

extern "C" {

int tmh_column_census_device(const double* dev_x, int64_t n, int d, const double* dev_center,
                             const double* dev_scale, int64_t* host_count, int64_t* host_inf,
                             double* host_mean, double* host_var, void* stream) {
  return guard([&] {
    census_dev(dev_x, n, d, dev_center, dev_scale, host_count, host_inf, host_mean, host_var, stream);
  });
}

int tmh_column_census(const double* host_x, int64_t n, int d, const double* host_center,
                      const double* host_scale, int64_t* host_count, int64_t* host_inf,
                      double* host_mean, double* host_var) {
  return guard([&] {
    HostTable t;
    t.upload(host_x, n, d, host_center, host_scale);
    census_dev(t.x.p, n, d, t.center.p, t.scale.p, host_count, host_inf, host_mean, host_var, nullptr);
  });
}

int tmh_column_select_device(const double* dev_x, int64_t n, int d, const int64_t* host_count,
                             const int64_t* host_ranks, int r, double* host_values, void* stream) {
  return guard([&] { select_dev(dev_x, n, d, host_count, host_ranks, r, host_values, stream); });
}

int tmh_column_select(const double* host_x, int64_t n, int d, const int64_t* host_count,
                      const int64_t* host_ranks, int r, double* host_values) {
  return guard([&] {
    HostTable t;
    t.upload(host_x, n, d, nullptr, nullptr);
    select_dev(t.x.p, n, d, host_count, host_ranks, r, host_values, nullptr);
  });
}

int tmh_robust_scale_device(const double* dev_x, int64_t n, int d, const double* dev_center,
                            const double* dev_scale, double* dev_out, void* stream) {
  return guard([&] { robust_scale_dev(dev_x, n, d, dev_center, dev_scale, dev_out, stream); });
}

int tmh_robust_scale(const double* host_x, int64_t n, int d, const double* host_center,
                     const double* host_scale, double* host_out) {
  return guard([&] {
    TMH_CHECK(host_center && host_scale && host_out, TMH_EINVAL,
              "center, scale or out pointer is NULL");
    HostTable t;
    t.upload(host_x, n, d, host_center, host_scale);
    DBuf<double> out;
    out.alloc((size_t)n * d);
    robust_scale_dev(t.x.p, n, d, t.center.p, t.scale.p, out.p, nullptr);
    TMH_HIP(hipStreamSynchronize(nullptr));
    out.download(host_out, (size_t)n * d);
  });
}

int tmh_kmeans_seed_device(const double* dev_x, int64_t n, int d, int k, const double* dev_center,
                           const double* dev_scale, int64_t first, const double* host_draws,
                           int trials, int32_t* host_indices, double* host_centers,
                           double* host_trace, void* stream) {
  return guard([&] {
    seed_dev(dev_x, n, d, k, dev_center, dev_scale, first, host_draws, trials, host_indices,
             host_centers, host_trace, stream);
  });
}

int tmh_kmeans_seed(const double* host_x, int64_t n, int d, int k, const double* host_center,
                    const double* host_scale, int64_t first, const double* host_draws, int trials,
                    int32_t* host_indices, double* host_centers, double* host_trace) {
  return guard([&] {
    check_kmeans(host_x, n, d, k);
    HostTable t;
    t.upload(host_x, n, d, host_center, host_scale);
    seed_dev(t.x.p, n, d, k, t.center.p, t.scale.p, first, host_draws, trials, host_indices,
             host_centers, host_trace, nullptr);
  });
}

int tmh_kmeans_predict_device(const double* dev_x, int64_t n, int d, int k, const double* dev_center,
                              const double* dev_scale, const double* host_centers,
                              int32_t* dev_labels, double* dev_min_dist, void* stream) {
  return guard([&] {
    predict_dev(dev_x, n, d, k, dev_center, dev_scale, host_centers, dev_labels, dev_min_dist,
                stream);
  });
}

int tmh_kmeans_predict(const double* host_x, int64_t n, int d, int k, const double* host_center,
                       const double* host_scale, const double* host_centers, int32_t* host_labels,
                       double* host_min_dist) {
  return guard([&] {
    check_kmeans(host_x, n, d, k, false);
    TMH_CHECK(host_labels, TMH_EINVAL, "labels pointer is NULL");
    HostTable t;
    t.upload(host_x, n, d, host_center, host_scale);
    DBuf<int32_t> lab;
    DBuf<double> md;
    lab.alloc((size_t)n);
    if (host_min_dist) md.alloc((size_t)n);
    predict_dev(t.x.p, n, d, k, t.center.p, t.scale.p, host_centers, lab.p, md.p, nullptr);
    lab.download(host_labels, (size_t)n);
    if (host_min_dist) md.download(host_min_dist, (size_t)n);
  });
}

int tmh_kmeans_fit_device(const double* dev_x, int64_t n, int d, int k, const double* dev_center,
                          const double* dev_scale, const double* host_init, int max_iter, double tol,
                          double* host_centers, int32_t* dev_labels, double* inertia, int* n_iter,
                          double* tol_abs, void* stream) {
  return guard([&] {
    fit_dev(dev_x, n, d, k, dev_center, dev_scale, host_init, max_iter, tol, host_centers,
            dev_labels, inertia, n_iter, tol_abs, stream);
  });
}

int tmh_kmeans_fit(const double* host_x, int64_t n, int d, int k, const double* host_center,
                   const double* host_scale, const double* host_init, int max_iter, double tol,
                   double* host_centers, int32_t* host_labels, double* inertia, int* n_iter,
                   double* tol_abs) {
  return guard([&] {
    check_kmeans(host_x, n, d, k);
    TMH_CHECK(host_labels, TMH_EINVAL, "labels pointer is NULL");
    HostTable t;
    t.upload(host_x, n, d, host_center, host_scale);
    DBuf<int32_t> lab;
    lab.alloc((size_t)n);
    fit_dev(t.x.p, n, d, k, t.center.p, t.scale.p, host_init, max_iter, tol, host_centers, lab.p,
            inertia, n_iter, tol_abs, nullptr);
    lab.download(host_labels, (size_t)n);
  });
}

}  // extern "C"
