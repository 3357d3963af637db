// Host build of tmlibrary_amd/csrc/classify_core.h: the validator, the packing,
// the forest's row walk and the SVC's pair accumulation, the code the
// classification kernels run, over records written by
// tests/test_classification_cpu.py.
//
//   classify_host <in> <out>
//
// in:  int32 count, then per record int32 kind (0 forest, 1 SVC) and
//   forest: int64 nodes, int32 n_trees, int64 n_leaves, int32 n_classes,
//           int32 d, int64 n; feature, threshold, left, right, leaf_row
//           [nodes], tree_root [n_trees], leaf_value [n_leaves][n_classes],
//           X [n][d]
//   SVC:    int32 kernel, f64 gamma, int64 m, int32 d, int32 k, int32
//           has_scaler, int32 tile, int64 n; sv [m][d], n_sv [k], coef
//           [k - 1][m], rho [pairs], (center, scale [d]), X [n][d]
// out: per record int32 status (0: ok, 1: the model was refused, 2: a row was
//   refused); when ok, labels int32 [n], then proba f64 [n][n_classes] or dec
//   f64 [n][pairs].  The SVC's support vectors are walked in tiles of `tile`
//   (0: all at once), as the kernel streams them.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define TMH_CHD inline
#include "../tmlibrary_amd/csrc/classify_core.h"

using namespace tmh;

static FILE* in;
static FILE* out;

template <typename T>
static std::vector<T> get(size_t count) {
  std::vector<T> v(count);
  if (count && fread(v.data(), sizeof(T), count, in) != count) {
    fprintf(stderr, "short read\n");
    exit(2);
  }
  return v;
}

template <typename T>
static T get1() {
  return get<T>(1)[0];
}

template <typename T>
static void put(const T* p, size_t count) {
  if (count && fwrite(p, sizeof(T), count, out) != count) {
    fprintf(stderr, "short write\n");
    exit(2);
  }
}

static void status(int32_t s) { put(&s, 1); }

static void forest_record() {
  const int64_t nodes = get1<int64_t>();
  const int32_t n_trees = get1<int32_t>();
  const int64_t n_leaves = get1<int64_t>();
  const int32_t C = get1<int32_t>(), d = get1<int32_t>();
  const int64_t n = get1<int64_t>();
  const auto feature = get<int32_t>((size_t)nodes);
  const auto threshold = get<double>((size_t)nodes);
  const auto left = get<int32_t>((size_t)nodes), right = get<int32_t>((size_t)nodes);
  const auto leaf_row = get<int32_t>((size_t)nodes);
  const auto roots = get<int32_t>((size_t)n_trees);
  const auto value = get<double>((size_t)(n_leaves * C));
  const auto X = get<double>((size_t)(n * d));
  const char* why =
      forest_validate(feature.data(), threshold.data(), left.data(), right.data(), leaf_row.data(),
                      nodes, roots.data(), n_trees, value.data(), n_leaves, C, d);
  std::vector<ForestNode> packed;
  std::vector<int32_t> proots;
  if (!why)
    why = forest_pack(feature.data(), threshold.data(), left.data(), right.data(), leaf_row.data(),
                      nodes, roots.data(), n_trees, packed, proots);
  if (why) {
    status(1);
    return;
  }
  for (double v : X)
    if (!(v - v == 0.0) || f32_cast_overflows(v)) {
      status(2);
      return;
    }
  std::vector<int32_t> labels((size_t)n), leaf((size_t)n_trees);
  std::vector<double> proba((size_t)(n * C));
  std::vector<float> x((size_t)d);
  for (int64_t r = 0; r < n; ++r) {
    for (int f = 0; f < d; ++f) x[(size_t)f] = (float)X[(size_t)(r * d + f)];
    for (int t = 0; t < n_trees; ++t)
      leaf[(size_t)t] = forest_leaf(packed.data(), proots[(size_t)t], x.data());
    double* p = proba.data() + r * C;
    for (int c = 0; c < C; ++c) p[c] = forest_class_proba(value.data(), leaf.data(), n_trees, C, c);
    labels[(size_t)r] = first_max(p, C);
  }
  status(0);
  put(labels.data(), labels.size());
  put(proba.data(), proba.size());
}

static void svc_record() {
  const int32_t kernel = get1<int32_t>();
  const double gamma = get1<double>();
  const int64_t m = get1<int64_t>();
  const int32_t d = get1<int32_t>(), k = get1<int32_t>(), has_scaler = get1<int32_t>();
  int32_t tile = get1<int32_t>();
  const int64_t n = get1<int64_t>();
  const int P = k * (k - 1) / 2;
  const auto sv = get<double>((size_t)(m * d));
  const auto n_sv = get<int32_t>((size_t)k);
  const auto coef = get<double>((size_t)((k - 1) * m));
  const auto rho = get<double>((size_t)P);
  std::vector<double> center, scale;
  if (has_scaler) {
    center = get<double>((size_t)d);
    scale = get<double>((size_t)d);
  }
  const auto X = get<double>((size_t)(n * d));
  if (svc_validate(kernel, gamma, sv.data(), m, d, n_sv.data(), k, coef.data(), rho.data())) {
    status(1);
    return;
  }
  for (double v : X)
    if (!(v - v == 0.0)) {
      status(2);
      return;
    }
  std::vector<int32_t> start((size_t)k + 1, 0);
  for (int c = 0; c < k; ++c) start[(size_t)c + 1] = start[(size_t)c] + n_sv[(size_t)c];
  std::vector<double> w;
  if (kernel == kSvcLinear) svc_collapse_linear(sv.data(), m, d, n_sv.data(), k, coef.data(), w);
  if (tile <= 0 || tile > m) tile = (int32_t)m;
  std::vector<int32_t> labels((size_t)n);
  std::vector<double> dec((size_t)(n * P)), x((size_t)d), K((size_t)tile);
  for (int64_t r = 0; r < n; ++r) {
    for (int f = 0; f < d; ++f) {
      const double v = X[(size_t)(r * d + f)];
      x[(size_t)f] = has_scaler ? (v - center[(size_t)f]) / scale[(size_t)f] : v;
    }
    double* dr = dec.data() + r * P;
    for (int p = 0; p < P; ++p) dr[p] = 0.0;
    if (kernel == kSvcLinear) {
      for (int p = 0; p < P; ++p)
        dr[p] = svc_kernel(kernel, gamma, x.data(), w.data() + (size_t)p * d, d);
    } else {
      for (int s0 = 0; s0 < m; s0 += tile) {
        const int s1 = s0 + tile < m ? s0 + tile : (int)m;
        for (int s = s0; s < s1; ++s)
          K[(size_t)(s - s0)] = svc_kernel(kernel, gamma, x.data(), sv.data() + (size_t)s * d, d);
        for (int i = 0; i < k; ++i)
          for (int j = i + 1; j < k; ++j) {
            double& a = dr[svc_pair_index(i, j, k)];
            a = svc_pair_accumulate(a, coef.data() + s0, m, K.data(), s0, s1, start.data(), i,
                                    j);
          }
      }
    }
    for (int p = 0; p < P; ++p) dr[p] -= rho[(size_t)p];
    labels[(size_t)r] = svc_vote(dr, 1, k);
  }
  status(0);
  put(labels.data(), labels.size());
  put(dec.data(), dec.size());
}

int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: classify_host <in> <out>\n");
    return 2;
  }
  in = fopen(argv[1], "rb");
  out = fopen(argv[2], "wb");
  if (!in || !out) {
    fprintf(stderr, "cannot open the files\n");
    return 2;
  }
  const int32_t count = get1<int32_t>();
  for (int32_t i = 0; i < count; ++i) {
    const int32_t kind = get1<int32_t>();
    if (kind == 0)
      forest_record();
    else
      svc_record();
  }
  fclose(in);
  return fclose(out) == 0 ? 0 : 2;
}
