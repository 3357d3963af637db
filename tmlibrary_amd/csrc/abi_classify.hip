// C-ABI of libtmhip.so (include/tmhip.h): the supervised classification tool --
// random-forest and SVC prediction from flat models.
#include <climits>
#include <cmath>

#include "abi_internal.h"
#include "classify_core.h"

struct tmh_forest {
  int d = 0, n_classes = 0, n_trees = 0;
  int nodes = 0;  // packed
  bool force_memory = false;
  DBuf<ForestNode> packed;
  DBuf<int32_t> roots;
  DBuf<double> leaf_value;
};

struct tmh_svc {
  int kernel = 0, d = 0, k = 0;
  int m = 0;  // rows of sv: the support vectors (rbf) or the pairs' weight vectors (linear)
  double gamma = 0.0;
  int tile_cap = 0;
  DBuf<double> sv, coef, rho;
  DBuf<int32_t> start;
};

namespace tmh {

static bool lds_route(const tmh_forest* h) { return !h->force_memory && forest_fits_lds(h->nodes); }

static void forest_predict_dev(tmh_forest* h, const double* dev_x, int64_t n, int32_t* dev_labels,
                               double* dev_proba, void* stream) {
  TMH_CHECK(h, TMH_EINVAL, "handle is NULL");
  check_table(dev_x, n, h->d);
  TMH_CHECK(dev_labels, TMH_EINVAL, "labels pointer is NULL");
  const size_t xb = (size_t)n * h->d * sizeof(double);
  const size_t pb = (size_t)n * h->n_classes * 8;
  TMH_CHECK(!overlap(dev_x, xb, dev_labels, (size_t)n * 4) &&
                (!dev_proba || !overlap(dev_x, xb, dev_proba, pb)),
            TMH_EINVAL, "input and output must not overlap");
  TMH_CHECK(!dev_proba || !overlap(dev_labels, (size_t)n * 4, dev_proba, pb), TMH_EINVAL,
            "the outputs must not overlap each other");
  hipStream_t s = (hipStream_t)stream;
  DBuf<unsigned long long> cnt, over;
  require_finite(dev_x, n, h->d, cnt, s);
  over.alloc(1);
  classify_count_f32_overflow(dev_x, n, h->d, over.p, s);
  unsigned long long n_over = 0;
  TMH_HIP(hipMemcpyAsync(&n_over, over.p, sizeof(n_over), hipMemcpyDeviceToHost, s));
  TMH_HIP(hipStreamSynchronize(s));
  TMH_CHECK(n_over == 0, TMH_EINVAL, "the data holds values too large for float32");
  forest_predict(dev_x, n, h->d, h->n_classes, h->n_trees, h->nodes, lds_route(h), h->packed.p,
                 h->roots.p, h->leaf_value.p, dev_labels, dev_proba, s);
  TMH_HIP(hipStreamSynchronize(s));
}

static void svc_predict_dev(tmh_svc* h, const double* dev_x, int64_t n, const double* dev_center,
                            const double* dev_scale, int32_t* dev_labels, double* dev_dec,
                            void* stream) {
  TMH_CHECK(h, TMH_EINVAL, "handle is NULL");
  check_table(dev_x, n, h->d);
  check_scaler(dev_center, dev_scale);
  TMH_CHECK(dev_labels, TMH_EINVAL, "labels pointer is NULL");
  const size_t xb = (size_t)n * h->d * sizeof(double);
  const size_t pairs = (size_t)h->k * (h->k - 1) / 2;
  TMH_CHECK(!overlap(dev_x, xb, dev_labels, (size_t)n * 4) &&
                (!dev_dec || !overlap(dev_x, xb, dev_dec, (size_t)n * pairs * 8)),
            TMH_EINVAL, "input and output must not overlap");
  TMH_CHECK(!dev_dec || !overlap(dev_labels, (size_t)n * 4, dev_dec, (size_t)n * pairs * 8),
            TMH_EINVAL, "the outputs must not overlap each other");
  hipStream_t s = (hipStream_t)stream;
  DBuf<unsigned long long> cnt;
  require_finite(dev_x, n, h->d, cnt, s);
  svc_predict(dev_x, n, h->d, h->k, h->kernel, h->gamma, h->m, h->tile_cap, dev_center, dev_scale,
              h->sv.p, h->coef.p, h->start.p, h->rho.p, dev_labels, dev_dec, s);
  TMH_HIP(hipStreamSynchronize(s));
}

}  // namespace tmh

extern "C" {

int tmh_forest_create(const int32_t* feature, const double* threshold, const int32_t* left,
                      const int32_t* right, const int32_t* leaf_row, int64_t nodes,
                      const int32_t* tree_root, int n_trees, const double* leaf_value,
                      int64_t n_leaves, int n_classes, int d, tmh_forest** out) {
  return guard([&] {
    TMH_CHECK(out, TMH_EINVAL, "out pointer is NULL");
    *out = nullptr;
    const char* why = forest_validate(feature, threshold, left, right, leaf_row, nodes, tree_root,
                                      n_trees, leaf_value, n_leaves, n_classes, d);
    TMH_CHECK(!why, TMH_EINVAL, why);
    std::vector<ForestNode> packed;
    std::vector<int32_t> roots;
    why = forest_pack(feature, threshold, left, right, leaf_row, nodes, tree_root, n_trees, packed,
                      roots);
    TMH_CHECK(!why, TMH_EINVAL, why);
    tmh_forest* h = new tmh_forest();
    try {
      h->d = d;
      h->n_classes = n_classes;
      h->n_trees = n_trees;
      h->nodes = (int)packed.size();
      h->packed.upload(packed.data(), packed.size());
      h->roots.upload(roots.data(), roots.size());
      h->leaf_value.upload(leaf_value, (size_t)n_leaves * n_classes);
    } catch (...) {
      delete h;
      throw;
    }
    *out = h;
  });
}

void tmh_forest_destroy(tmh_forest* h) { delete h; }

int tmh_forest_set_option(tmh_forest* h, int option, int value) {
  return guard([&] {
    TMH_CHECK(h, TMH_EINVAL, "handle is NULL");
    TMH_CHECK(option == TMH_OPT_FOREST_MEMORY_ROUTE, TMH_EINVAL, "unknown option");
    TMH_CHECK(value == 0 || value == 1, TMH_EINVAL, "the memory route is 0 or 1");
    h->force_memory = value != 0;
  });
}

int tmh_forest_route(const tmh_forest* h, int* route, int64_t* packed_nodes) {
  return guard([&] {
    TMH_CHECK(h && route, TMH_EINVAL, "handle or route pointer is NULL");
    *route = lds_route(h) ? TMH_FOREST_ROUTE_LDS : TMH_FOREST_ROUTE_MEMORY;
    if (packed_nodes) *packed_nodes = h->nodes;
  });
}

int tmh_forest_predict_device(tmh_forest* h, const double* dev_x, int64_t n, int32_t* dev_labels,
                              double* dev_proba, void* stream) {
  return guard([&] { forest_predict_dev(h, dev_x, n, dev_labels, dev_proba, stream); });
}

int tmh_forest_predict(tmh_forest* h, const double* host_x, int64_t n, int32_t* host_labels,
                       double* host_proba) {
  return guard([&] {
    TMH_CHECK(h, TMH_EINVAL, "handle is NULL");
    TMH_CHECK(host_labels, TMH_EINVAL, "labels pointer is NULL");
    HostTable t;
    t.upload(host_x, n, h->d, nullptr, nullptr);
    DBuf<int32_t> lab;
    DBuf<double> pr;
    lab.alloc((size_t)n);
    if (host_proba) pr.alloc((size_t)n * h->n_classes);
    forest_predict_dev(h, t.x.p, n, lab.p, pr.p, nullptr);
    lab.download(host_labels, (size_t)n);
    if (host_proba) pr.download(host_proba, (size_t)n * h->n_classes);
  });
}

int tmh_svc_create(int kernel, double gamma, const double* sv, int64_t m, int d, const int32_t* n_sv,
                   int k, const double* coef, const double* rho, tmh_svc** out) {
  return guard([&] {
    TMH_CHECK(out, TMH_EINVAL, "out pointer is NULL");
    *out = nullptr;
    const char* why = svc_validate(kernel, gamma, sv, m, d, n_sv, k, coef, rho);
    TMH_CHECK(!why, TMH_EINVAL, why);
    tmh_svc* h = new tmh_svc();
    try {
      h->kernel = kernel;
      h->d = d;
      h->k = k;
      h->gamma = gamma;
      h->rho.upload(rho, (size_t)k * (k - 1) / 2);
      if (kernel == TMH_SVC_LINEAR) {
        std::vector<double> w;
        svc_collapse_linear(sv, m, d, n_sv, k, coef, w);
        for (double v : w)
          TMH_CHECK(std::isfinite(v), TMH_EINVAL, "a pair's weight vector is not finite");
        h->m = k * (k - 1) / 2;
        h->sv.upload(w.data(), w.size());
      } else {
        std::vector<int32_t> start((size_t)k + 1, 0);
        for (int c = 0; c < k; ++c) start[(size_t)c + 1] = start[(size_t)c] + n_sv[c];
        h->m = (int)m;
        h->sv.upload(sv, (size_t)m * d);
        h->coef.upload(coef, (size_t)(k - 1) * m);
        h->start.upload(start.data(), start.size());
      }
    } catch (...) {
      delete h;
      throw;
    }
    *out = h;
  });
}

void tmh_svc_destroy(tmh_svc* h) { delete h; }

int tmh_svc_set_option(tmh_svc* h, int option, int value) {
  return guard([&] {
    TMH_CHECK(h, TMH_EINVAL, "handle is NULL");
    TMH_CHECK(option == TMH_OPT_SVC_TILE, TMH_EINVAL, "unknown option");
    TMH_CHECK(value >= 0 && value <= TMH_SVC_MAX_SV, TMH_EINVAL,
              "the tile cap is 0 (none) .. 65,536 support vectors");
    h->tile_cap = value;
  });
}

int tmh_svc_tile(const tmh_svc* h, int* tile, int* n_tiles) {
  return guard([&] {
    TMH_CHECK(h && tile, TMH_EINVAL, "handle or tile pointer is NULL");
    *tile = svc_tile_svs(h->d, h->k, h->kernel, h->m, h->tile_cap);
    if (n_tiles) *n_tiles = (h->m + *tile - 1) / *tile;
  });
}

int tmh_svc_predict_device(tmh_svc* h, const double* dev_x, int64_t n, const double* dev_center,
                           const double* dev_scale, int32_t* dev_labels, double* dev_dec,
                           void* stream) {
  return guard(
      [&] { svc_predict_dev(h, dev_x, n, dev_center, dev_scale, dev_labels, dev_dec, stream); });
}

int tmh_svc_predict(tmh_svc* h, const double* host_x, int64_t n, const double* host_center,
                    const double* host_scale, int32_t* host_labels, double* host_dec) {
  return guard([&] {
    TMH_CHECK(h, TMH_EINVAL, "handle is NULL");
    TMH_CHECK(host_labels, TMH_EINVAL, "labels pointer is NULL");
    HostTable t;
    t.upload(host_x, n, h->d, host_center, host_scale);
    const size_t pairs = (size_t)h->k * (h->k - 1) / 2;
    DBuf<int32_t> lab;
    DBuf<double> dec;
    lab.alloc((size_t)n);
    if (host_dec) dec.alloc((size_t)n * pairs);
    svc_predict_dev(h, t.x.p, n, t.center.p, t.scale.p, lab.p, dec.p, nullptr);
    lab.download(host_labels, (size_t)n);
    if (host_dec) dec.download(host_dec, (size_t)n * pairs);
  });
}

}  // extern "C"
