// The supervised classification tool's row rules (tmlib/tools/classification.py
// through Classifier.predict, tmlib/tools/base.py:621-645): what scikit-learn's
// RandomForestClassifier.predict and libsvm's dense svm_predict_values compute
// for one row, and the checks a flat model passes before it is used.  Kept free
// of HIP headers so that the code k_forest_predict and k_svc_predict run
// (classify_kernels.hip) also builds for the host (tests/classify_host.cpp).
// DESIGN.md section 23.
//
// Forest.  A row is cast to f32; at a node it goes left iff
// (double)x_f32[feature] <= threshold; a leaf gives its row of fractions; the
// trees' rows are added in f64 in tree order into zero, each class sum is
// divided by n_trees once, the label is the first maximum.
//
// SVC.  K_s = exp(-gamma sum_f (x_f - sv_sf)^2) (rbf) or x . sv_s (linear), in
// feature order with fused multiply-adds; for a pair (i < j), in libsvm's pair
// order, dec = sum over the SVs of i of coef[j - 1][s] K_s + the SVs of j of
// coef[i][s] K_s, in ascending s with fused multiply-adds, then - rho[p]; the
// vote goes to i iff dec > 0; the label is the first class with the most votes.
#pragma once

#include <cmath>
#include <cstdint>
#include <vector>

#ifndef TMH_CHD
#define TMH_CHD __host__ __device__ __forceinline__
#endif

namespace tmh {

// the limits of include/tmhip.h, restated for the host build
constexpr int kClassifyMaxD = 256;
constexpr int kForestMaxClasses = 64;
constexpr int kForestMaxTrees = 256;
constexpr int64_t kForestMaxNodes = (int64_t)1 << 24;
constexpr int kSvcMaxClasses = 16;
constexpr int64_t kSvcMaxSv = 65536;
constexpr int kSvcRbf = 0, kSvcLinear = 1;

// A packed node.  Trees are renumbered in preorder, so an internal node's left
// child is the next node and `next` is its right child; a leaf has feature -1
// and `next` is its row of leaf_value.  Every `next` of an internal node is
// greater than the node's own index: a walk ends.
struct ForestNode {
  double threshold;
  int32_t feature;
  int32_t next;
};

namespace {

// the leaf row a row of f32 features ends in
TMH_CHD int forest_leaf(const ForestNode* nodes, int root, const float* x) {
  int i = root;
  for (;;) {
    const ForestNode nd = nodes[i];
    if (nd.feature < 0) return nd.next;
    i = ((double)x[nd.feature] <= nd.threshold) ? i + 1 : nd.next;
  }
}

// class c's probability from the trees' leaf rows: adds in tree order into
// zero, one divide
TMH_CHD double forest_class_proba(const double* leaf_value, const int32_t* leaf_of_tree,
                                  int n_trees, int n_classes, int c) {
  double a = 0.0;
  for (int t = 0; t < n_trees; ++t) a += leaf_value[(int64_t)leaf_of_tree[t] * n_classes + c];
  return a / (double)n_trees;
}

TMH_CHD int first_max(const double* p, int n) {
  int best = 0;
  for (int c = 1; c < n; ++c)
    if (p[c] > p[best]) best = c;
  return best;
}

// a finite f64 whose f32 cast (round to nearest even) is infinite
TMH_CHD bool f32_cast_overflows(double v) {
  const float f = (float)v;
  return v - v == 0.0 && f - f != 0.0f;
}

TMH_CHD double svc_kernel(int kernel, double gamma, const double* x, const double* sv, int d) {
  double a = 0.0;
  if (kernel == kSvcRbf) {
    for (int f = 0; f < d; ++f) {
      const double t = x[f] - sv[f];
      a = fma(t, t, a);
    }
    return exp(-gamma * a);
  }
  for (int f = 0; f < d; ++f) a = fma(x[f], sv[f], a);
  return a;
}

// libsvm's pair order: (0,1), (0,2), ..., (0,k-1), (1,2), ...
TMH_CHD int svc_pair_index(int i, int j, int k) { return i * (2 * k - i - 1) / 2 + (j - i - 1); }

// dec of pair (i, j) continued over the SVs [s0, s1) of the model; K[s - s0]
// their kernel values and coef[row * coef_stride + s - s0] their coefficients
// (both hold the tile's columns only); start[c] the first SV of class c
// (start[k] = m)
TMH_CHD double svc_pair_accumulate(double acc, const double* coef, int64_t coef_stride,
                                   const double* K, int s0, int s1, const int32_t* start, int i,
                                   int j) {
  int a = start[i] > s0 ? start[i] : s0, b = start[i + 1] < s1 ? start[i + 1] : s1;
  for (int s = a; s < b; ++s)
    acc = fma(coef[(int64_t)(j - 1) * coef_stride + s - s0], K[s - s0], acc);
  a = start[j] > s0 ? start[j] : s0;
  b = start[j + 1] < s1 ? start[j + 1] : s1;
  for (int s = a; s < b; ++s) acc = fma(coef[(int64_t)i * coef_stride + s - s0], K[s - s0], acc);
  return acc;
}

// the label from the pairs' decision values (rho already subtracted)
TMH_CHD int svc_vote(const double* dec, int64_t dec_stride, int k) {
  // 16 classes of at most 15 votes each: 4 bits per class
  uint64_t votes = 0;
  int p = 0;
  for (int i = 0; i < k; ++i)
    for (int j = i + 1; j < k; ++j, ++p) votes += 1ull << (4 * (dec[p * dec_stride] > 0.0 ? i : j));
  int best = 0, bv = (int)(votes & 15u);
  for (int c = 1; c < k; ++c) {
    const int v = (int)((votes >> (4 * c)) & 15u);
    if (v > bv) {
      bv = v;
      best = c;
    }
  }
  return best;
}

}  // namespace

// What tmh_forest_create checks; nullptr when the model is sound, else the
// message.  Tree t owns the nodes [tree_root[t], tree_root[t + 1]) (the last
// tree: up to `nodes`).
inline const char* forest_validate(const int32_t* feature, const double* threshold,
                                   const int32_t* left, const int32_t* right,
                                   const int32_t* leaf_row, int64_t nodes, const int32_t* tree_root,
                                   int n_trees, const double* leaf_value, int64_t n_leaves,
                                   int n_classes, int d) {
  if (d < 1 || d > kClassifyMaxD) return "d is over the limit of 256 features";
  if (n_classes < 2 || n_classes > kForestMaxClasses) return "n_classes must be 2 .. 64";
  if (n_trees < 1 || n_trees > kForestMaxTrees) return "n_trees must be 1 .. 256";
  if (nodes < 1 || nodes >= kForestMaxNodes) return "nodes must be 1 .. 2^24 - 1";
  if (n_leaves < 1 || n_leaves > nodes) return "n_leaves must be 1 .. nodes";
  if (!feature || !threshold || !left || !right || !leaf_row || !tree_root || !leaf_value)
    return "a model pointer is NULL";
  if (tree_root[0] != 0) return "the first tree must start at node 0";
  for (int t = 0; t < n_trees; ++t) {
    const int64_t lo = tree_root[t], hi = t + 1 < n_trees ? (int64_t)tree_root[t + 1] : nodes;
    if (lo < 0 || lo >= hi || hi > nodes) return "tree roots must ascend inside the nodes";
    for (int64_t i = lo; i < hi; ++i) {
      if (feature[i] == -1) {
        if (leaf_row[i] < 0 || leaf_row[i] >= n_leaves) return "a leaf row is out of range";
        continue;
      }
      if (feature[i] < 0 || feature[i] >= d) return "a node's feature is not below d";
      if (threshold[i] != threshold[i]) return "a threshold is NaN";
      if (left[i] >= hi || right[i] >= hi || left[i] < lo || right[i] < lo)
        return "a child lies outside its tree";
      if (left[i] <= i || right[i] <= i) return "a child's index is not greater than its parent's";
    }
  }
  for (int64_t i = 0; i < n_leaves * n_classes; ++i)
    if (!(leaf_value[i] - leaf_value[i] == 0.0)) return "a leaf value is not finite";
  return nullptr;
}

// The packed forest of a validated model: per tree the nodes its root reaches,
// in preorder.  nullptr, or the message when a node is reached twice.
inline const char* forest_pack(const int32_t* feature, const double* threshold, const int32_t* left,
                               const int32_t* right, const int32_t* leaf_row, int64_t nodes,
                               const int32_t* tree_root, int n_trees, std::vector<ForestNode>& packed,
                               std::vector<int32_t>& roots) {
  packed.clear();
  roots.assign((size_t)n_trees, 0);
  std::vector<char> seen((size_t)nodes, 0);
  std::vector<int32_t> stack, parent;  // nodes to visit; the packed parent whose right child each is
  for (int t = 0; t < n_trees; ++t) {
    roots[(size_t)t] = (int32_t)packed.size();
    stack.assign(1, tree_root[t]);
    parent.assign(1, -1);
    while (!stack.empty()) {
      const int32_t i = stack.back(), from = parent.back();
      stack.pop_back();
      parent.pop_back();
      if (seen[(size_t)i]) return "a node is reached twice";
      seen[(size_t)i] = 1;
      const int32_t at = (int32_t)packed.size();
      if (from >= 0) packed[(size_t)from].next = at;
      if (feature[i] == -1) {
        packed.push_back(ForestNode{0.0, -1, leaf_row[i]});
        continue;
      }
      packed.push_back(ForestNode{threshold[i], feature[i], 0});
      stack.push_back(right[i]);  // visited after the whole left subtree
      parent.push_back(at);
      stack.push_back(left[i]);   // next: lands at `at + 1`
      parent.push_back(-1);
    }
  }
  return nullptr;
}

// What tmh_svc_create checks.  sv [m][d], n_sv [k], coef [k - 1][m], rho [k (k - 1) / 2].
inline const char* svc_validate(int kernel, double gamma, const double* sv, int64_t m, int d,
                                const int32_t* n_sv, int k, const double* coef, const double* rho) {
  if (kernel != kSvcRbf && kernel != kSvcLinear) return "kernel must be rbf or linear";
  if (d < 1 || d > kClassifyMaxD) return "d is over the limit of 256 features";
  if (k < 2 || k > kSvcMaxClasses) return "k must be 2 .. 16 classes";
  if (m < 1 || m > kSvcMaxSv) return "m must be 1 .. 65,536 support vectors";
  if (!sv || !n_sv || !coef || !rho) return "a model pointer is NULL";
  if (kernel == kSvcRbf && !(gamma > 0.0 && gamma - gamma == 0.0))
    return "gamma must be positive and finite";
  int64_t total = 0;
  for (int c = 0; c < k; ++c) {
    if (n_sv[c] < 0) return "a class has a negative number of support vectors";
    total += n_sv[c];
  }
  if (total != m) return "n_sv does not add up to m";
  for (int64_t i = 0; i < m * d; ++i)
    if (!(sv[i] - sv[i] == 0.0)) return "a support vector is not finite";
  for (int64_t i = 0; i < (int64_t)(k - 1) * m; ++i)
    if (!(coef[i] - coef[i] == 0.0)) return "a coefficient is not finite";
  for (int p = 0; p < k * (k - 1) / 2; ++p)
    if (!(rho[p] - rho[p] == 0.0)) return "rho is not finite";
  return nullptr;
}

// The linear kernel collapsed: w[p][f] = sum over the pair's SVs, in ascending
// s, of coef_s sv_sf, so that dec = x . w[p] - rho[p].
inline void svc_collapse_linear(const double* sv, int64_t m, int d, const int32_t* n_sv, int k,
                                const double* coef, std::vector<double>& w) {
  std::vector<int32_t> start((size_t)k + 1, 0);
  for (int c = 0; c < k; ++c) start[(size_t)c + 1] = start[(size_t)c] + n_sv[c];
  w.assign((size_t)(k * (k - 1) / 2) * d, 0.0);
  int p = 0;
  for (int i = 0; i < k; ++i)
    for (int j = i + 1; j < k; ++j, ++p)
      for (int f = 0; f < d; ++f) {
        double a = 0.0;
        for (int s = start[(size_t)i]; s < start[(size_t)i + 1]; ++s)
          a = std::fma(coef[(int64_t)(j - 1) * m + s], sv[(int64_t)s * d + f], a);
        for (int s = start[(size_t)j]; s < start[(size_t)j + 1]; ++s)
          a = std::fma(coef[(int64_t)i * m + s], sv[(int64_t)s * d + f], a);
        w[(size_t)p * d + f] = a;
      }
}

}  // namespace tmh
